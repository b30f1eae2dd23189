// opental_amd/csrc/openmax.hip -- the OpenMax baseline on gfx950 (AFSD/thumos14/openmax.py, test_openmax.py):
//   otal_openmax_dist        : eucos distances of feature rows against class mean activation vectors (MAVs)
//                              (openmax.py:7-9, test_openmax.py:319,324);
//   otal_openmax_class_means : per-class mean of labelled feature rows (test_openmax.py:317-318,322-323);
//   otal_openmax_probs       : OpenMax.forward (openmax.py:42-86) for N rows in one launch;
//   otal_decode_clips_openmax: decode_output + the threshold test of `filtering` (test_openmax.py:141-189) for a batch of
//                              clips in one launch -- both stages' recalibration, their average, the centre factor, the
//                              segments and flag = score > conf_thresh; no (N, K + 1) intermediate goes to memory.
// The reference copies logits and features to the host and loops in Python over every anchor and class with two scipy
// calls and a libMR call each, twice per clip.
//
// One tile kernel serves dist / probs / decode.  A workgroup of 256 threads owns 16 feature rows: the MAVs of every stage
// (K x D floats each, 30 KB at K = 15, D = 512) and the 16 rows are staged into LDS once -- every feature element is read
// from memory exactly once, with the thread -> element mapping chosen by which feature stride is the unit one, so that both
// the (B, A, D) copy and a permuted view of the channel-major (B, D, A) map are read coalesced and in place.  LDS rows are
// padded by 4 floats: the 16 class rows (and the 4 feature rows) a wave's ds_read_b128 touches then fall on distinct
// banks.  Thread (r, j) = (row, class slot) walks the D channels in order d = 0 .. D-1 with fp32 partial sums (f.f, f.m, m.m,
// |f - m|^2; see Sums): a fixed order that does not depend on the memory layout, so both layouts give the same bits.
// The 16 lanes of a row then hold its K distances; ranks, the sums over classes and the softmax run on 16-lane shuffles
// (xor butterfly: fixed order again).
//
// w-score.  libMR evaluates 1 - exp(-((d + 10000 - small) / scale) ^ shape) in double.  In fp32 `d + 10000 - small` has an
// ulp of 1e-3 and shape is of order 1e5, so the literal form is off by 2e-3 in w.  The host passes per class, prepared in
// float64, off = small + (scale - 10000), inv_scale = 1 / scale and shape; with u = (d - off) * inv_scale the translated
// argument over scale is 1 + u, and  w = -expm1(-exp(shape * log1p(u))),  w = 0 where 1 + u <= 0 (weibull_cdf, weibull.c:79-104).
#include "openmax_common.h"       // OmxArgs, FeatView, stage_feat, w_score, omx_tile, omx_launch and the argument checks:
                                  // shared with csrc/openmax_wide.hip

namespace {

constexpr int OMX_KS = 16;            // class slots per row (K <= 16)
static_assert(OMX_THREADS == OMX_TR * OMX_KS, "one thread per (row, class slot)");
constexpr int CM_GROUPS = 16;         // row groups (waves) of a class-means workgroup

// (K, D) contiguous, 16-byte aligned (checked by the entry points) -> s[k * ld + d]
__device__ void stage_mav(float* s, int ld, const float* mav, int K, int D) {
    const int q4 = D >> 2, total = K * q4;
#pragma unroll 4
    for (int i = threadIdx.x; i < total; i += OMX_THREADS) {
        const int k = i / q4, q = i - k * q4;
        *reinterpret_cast<float4*>(s + k * ld + 4 * q) = *reinterpret_cast<const float4*>(mav + (size_t)k * D + 4 * q);
    }
}

// f.f, f.m, m.m and |f - m|^2 over the D channels.  The cosine term 1 - f.m / (|f| |m|) is a small difference of numbers near
// 1, so the three dot products carry its whole error: each runs on 16 partial sums (channel d goes to partial d % 16, 32
// terms each at D = 512) that a fixed tree adds at the end -- the error of numpy's pairwise sum rather than that of one
// 512-term chain (measured on the 600 x 15 distances of the fixture: 1.5e-6 with one accumulator per sum).  The euclidean
// term is divided by 200 and keeps 4 partial sums.
struct Sums { float ff[16], fm[16], mm[16], ee[4]; };

__device__ __forceinline__ void sums_clear(Sums& s) {
#pragma unroll
    for (int i = 0; i < 16; ++i) s.ff[i] = s.fm[i] = s.mm[i] = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) s.ee[i] = 0.f;
}

__device__ __forceinline__ void acc1(Sums& s, int i, float a, float b) {
    s.ff[i] = fmaf(a, a, s.ff[i]);
    s.fm[i] = fmaf(a, b, s.fm[i]);
    s.mm[i] = fmaf(b, b, s.mm[i]);
    const float e = a - b;
    s.ee[i & 3] = fmaf(e, e, s.ee[i & 3]);
}

// channels 16 * q16 .. 16 * q16 + 15
__device__ __forceinline__ void acc16(Sums& s, const float4* f, const float4* m, int q16) {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const float4 a = f[4 * q16 + p], b = m[4 * q16 + p];
        acc1(s, 4 * p, a.x, b.x); acc1(s, 4 * p + 1, a.y, b.y); acc1(s, 4 * p + 2, a.z, b.z); acc1(s, 4 * p + 3, a.w, b.w);
    }
}

__device__ __forceinline__ float tree16(const float* v) {
    float t[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) t[i] = v[2 * i] + v[2 * i + 1];
    return ((t[0] + t[1]) + (t[2] + t[3])) + ((t[4] + t[5]) + (t[6] + t[7]));
}

// compute_eucos_dist (openmax.py:7-9): euclidean / 200 + (1 - cosine similarity)
__device__ __forceinline__ float eucos(const Sums& s) {
    const float ee = (s.ee[0] + s.ee[1]) + (s.ee[2] + s.ee[3]);
    return sqrtf(ee) / 200.0f + (1.0f - tree16(s.fm) / (sqrtf(tree16(s.ff)) * sqrtf(tree16(s.mm))));
}

// openmax_recalibrate + compute_openmax_prob (openmax.py:21-73) for one row, one lane per class slot j of a 16-lane group
// (lanes j >= K idle but take part in the shuffles).  z: this lane's logit, d: its distance.  Returns P(class j); P(unknown)
// in `pu` on every lane.  The i-th largest logit (i = 1 .. R) gets alpha = (R + 1 - i) / R; equal logits rank the HIGHER
// index first, which is what `argsort()[::-1]` gives.  The softmax over the K + 1 exponents subtracts their maximum (the
// reference does not: same value, no overflow).
__device__ __forceinline__ float openmax_recalibrate(float z, float d, const float* wb, int K, int R, int j, float& pu) {
    const bool valid = j < K;
    int rank = 0;
    for (int c = 0; c < K; ++c) {
        const float l = __shfl(z, c, OMX_KS);
        rank += (l > z) || (l == z && c > j);
    }
    const float alpha = rank < R ? (float)(R - rank) / (float)R : 0.f;
    const float w = w_score(d, wb);
    float mod = z * (1.0f - w * alpha);
    float unk = z - mod;
    if (!valid) { mod = -INFINITY; unk = 0.f; }
    float su = unk, mx = mod;
#pragma unroll
    for (int o = OMX_KS / 2; o > 0; o >>= 1) {
        su += __shfl_xor(su, o, OMX_KS);
        mx = fmaxf(mx, __shfl_xor(mx, o, OMX_KS));
    }
    mx = fmaxf(mx, su);
    const float e = valid ? expf(mod - mx) : 0.f;
    const float eu = expf(su - mx);
    float se = e;
#pragma unroll
    for (int o = OMX_KS / 2; o > 0; o >>= 1) se += __shfl_xor(se, o, OMX_KS);
    const float den = se + eu;
    pu = eu / den;
    return e / den;
}

// MODE 0: dist (N, K); 1: dist (N,) of each row against the class of its label; 2: probs (N, K + 1); 3: decode.
template <int MODE>
__global__ __launch_bounds__(OMX_THREADS) void openmax_tile_kernel(OmxArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int NS = MODE == 3 ? 2 : 1;
    const int K = a.K, D = a.D, ld = D + OMX_PAD;
    float* sM0 = reinterpret_cast<float*>(smem);
    float* sM1 = sM0 + (NS - 1) * K * ld;
    float* sF0 = sM0 + NS * K * ld;
    float* sF1 = (NS == 2 && a.two_feats) ? sF0 + OMX_TR * ld : sF0;
    int n0, nvalid, clip, row0;
    omx_tile<MODE == 3>(a, n0, nvalid, clip, row0);
    stage_mav(sM0, ld, a.mav0, K, D);
    stage_feat(sF0, ld, a.f0, n0, nvalid, D);
    if constexpr (NS == 2) {
        stage_mav(sM1, ld, a.mav1, K, D);
        if (a.two_feats) stage_feat(sF1, ld, a.f1, n0, nvalid, D);
    }
    __syncthreads();
    const int r = threadIdx.x / OMX_KS, j = threadIdx.x % OMX_KS, jc = min(j, K - 1);
    const float4* f0 = reinterpret_cast<const float4*>(sF0 + r * ld);
    const float4* f1 = reinterpret_cast<const float4*>(sF1 + r * ld);
    const float4* m0 = reinterpret_cast<const float4*>(sM0 + jc * ld);
    const float4* m1 = reinterpret_cast<const float4*>(sM1 + jc * ld);
    Sums s0, s1;
    sums_clear(s0);
    sums_clear(s1);
    const int q16 = D >> 4;
    for (int q = 0; q < q16; ++q) {
        acc16(s0, f0, m0, q);
        if constexpr (NS == 2) acc16(s1, f1, m1, q);
    }
    const bool rv = r < nvalid, live = rv && j < K;
    const int n = n0 + r;
    const float d0 = eucos(s0);
    if constexpr (MODE == 0) {
        if (live) a.out[(size_t)n * K + j] = d0;
    } else if constexpr (MODE == 1) {
        if (rv) {
            const int lab = a.labels[n];
            if (lab >= 0 && lab < K) { if (j == lab) a.out[n] = d0; }
            else if (j == 0) a.out[n] = -1.0f;
        }
    } else if constexpr (MODE == 2) {
        const float z = live ? a.logit0[(long long)n * a.ldl + j] : 0.f;
        float pu;
        const float p = openmax_recalibrate(z, d0, a.wb0 + jc * 3, K, a.R, j, pu);
        if (live) a.out[(size_t)n * (K + 1) + 1 + j] = p;
        if (rv && j == 0) a.out[(size_t)n * (K + 1)] = pu;
    } else {
        const float d1 = eucos(s1);
        const float z0 = live ? a.logit0[(long long)n * a.ldl + j] : 0.f;
        const float z1 = live ? a.logit1[(long long)n * a.ldl + j] : 0.f;
        float pu0, pu1;
        const float p0 = openmax_recalibrate(z0, d0, a.wb0 + jc * 3, K, a.R, j, pu0);
        const float p1 = openmax_recalibrate(z1, d1, a.wb1 + jc * 3, K, a.R, j, pu1);
        if (rv) {
            const int i = row0 + r;
            const float ct = omx_sigmoid(a.center[n]);
            if (j < K) {
                const size_t o = ((size_t)clip * K + j) * a.A + i;
                const float sc = (p0 + p1) / 2.0f * ct;             // test_openmax.py:162-163
                a.score[o] = sc;
                a.flag[o] = sc > a.conf_thresh;                     // filtering, test_openmax.py:174
            }
            if (j == 0) {
                a.unknown[n] = (pu0 + pu1) / 2.0f * ct;
                // late fusion + segments (test_openmax.py:150-156)
                decode_segment(a.loc, a.prop_loc, a.priors, a.offsets, a.fps, a.seg, n, i, clip, a.clip_length);
            }
        }
    }
}

// One workgroup per (class, 64 channels); wave g sums rows g, g + 16, ... of its class in row order, then the 16 partial
// sums are added in the order g = 0 .. 15: a fixed order and no atomics, so two runs give the same bits.
__global__ __launch_bounds__(CM_GROUPS * 64) void class_means_kernel(FeatView f, const int* __restrict__ labels, int N, int K,
                                                                      int D, float* __restrict__ means, int* __restrict__ counts) {
    __shared__ float part[CM_GROUPS][64];
    __shared__ int cnt[CM_GROUPS];
    const int k = blockIdx.x, lane = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int c = blockIdx.y * 64 + lane;
    float s = 0.f;
    int m = 0;
    for (int n = g; n < N; n += 4 * CM_GROUPS) {
        float v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int nn = n + u * CM_GROUPS;
            const bool hit = nn < N && labels[nn] == k;         // wave-uniform
            m += hit;
            v[u] = (hit && c < D) ? feat_row(f, nn)[(long long)c * f.sc] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) s += v[u];
    }
    part[g][lane] = s;
    if (lane == 0) cnt[g] = m;
    __syncthreads();
    if (g == 0) {
        float tot = 0.f;
        int ct = 0;
        for (int i = 0; i < CM_GROUPS; ++i) { tot += part[i][lane]; ct += cnt[i]; }
        if (c < D) means[(size_t)k * D + c] = ct > 0 ? tot / (float)ct : 0.f;
        if (blockIdx.y == 0 && lane == 0) counts[k] = ct;
    }
}

template <int MODE>
int launch_tile(const OmxArgs& a, int blocks, void* stream) {
    constexpr int stages = MODE == 3 ? 2 : 1;
    const size_t lds = (size_t)(stages * a.K + (1 + (stages == 2 && a.two_feats)) * OMX_TR) * (a.D + OMX_PAD) * sizeof(float);
    return omx_launch<openmax_tile_kernel<MODE>>(a, blocks, lds, stream);
}

}  // namespace

extern "C" int otal_openmax_dist(const float* feat, int N, int rows_per_batch, int64_t sb, int64_t sr, int64_t sc,
                                 const float* mav, int K, int D, const int* labels, float* dist, void* stream) {
    if (!feat || !mav || !dist) return OTAL_E_NULL;
    OmxArgs a;
    if (int e = omx_rows_args(feat, N, rows_per_batch, sb, sr, sc, mav, K, D, 1, K, OMX_KS, a)) return e;
    a.labels = labels; a.out = dist;
    return labels ? launch_tile<1>(a, omx_tiles(N), stream) : launch_tile<0>(a, omx_tiles(N), stream);
}

extern "C" int otal_openmax_class_means(const float* feat, int N, int rows_per_batch, int64_t sb, int64_t sr, int64_t sc,
                                        const int* labels, int K, int D, float* means, int* counts, void* stream) {
    if (!feat || !labels || !means || !counts) return OTAL_E_NULL;
    if (N <= 0 || rows_per_batch <= 0 || K <= 0 || D <= 0) return OTAL_E_SHAPE;
    const FeatView f{feat, rows_per_batch, (long long)sb, (long long)sr, (long long)sc};
    hipLaunchKernelGGL(class_means_kernel, dim3(K, (D + 63) / 64), dim3(CM_GROUPS * 64), 0, (hipStream_t)stream, f, labels, N,
                       K, D, means, counts);
    return otal_launch_status();
}

extern "C" int otal_openmax_probs(const float* logits, int64_t ldl, const float* feat, int N, int rows_per_batch, int64_t sb,
                                  int64_t sr, int64_t sc, const float* mav, const float* wb, int K, int D, int R,
                                  float* probs, void* stream) {
    if (!logits || !feat || !mav || !wb || !probs) return OTAL_E_NULL;
    OmxArgs a;
    if (int e = omx_rows_args(feat, N, rows_per_batch, sb, sr, sc, mav, K, D, R, ldl, OMX_KS, a)) return e;
    a.wb0 = wb; a.logit0 = logits; a.out = probs;
    return launch_tile<2>(a, omx_tiles(N), stream);
}

extern "C" int otal_decode_clips_openmax(const float* loc, const float* prop_loc, const float* priors, const float* conf,
                                         const float* prop_conf, const float* center, const float* offsets,
                                         const float* fps, const float* feat, const float* prop_feat,
                                         const int64_t* feat_strides, const int64_t* prop_feat_strides, const float* mav,
                                         const float* mav_prop, const float* wb, const float* wb_prop, float* seg,
                                         float* score, float* unknown, unsigned char* flag, int nclips, int A, int C,
                                         int first_class, int D, int R, int refined_feature, float clip_length,
                                         float conf_thresh, void* stream) {
    OmxArgs a;
    if (int e = omx_decode_args(loc, prop_loc, priors, conf, prop_conf, center, offsets, fps, feat, prop_feat, feat_strides,
                                prop_feat_strides, mav, mav_prop, wb, wb_prop, seg, score, unknown, flag, nclips, A, C,
                                first_class, D, R, refined_feature, clip_length, conf_thresh, OMX_KS, a))
        return e;
    return launch_tile<3>(a, nclips * omx_tiles(A), stream);
}

