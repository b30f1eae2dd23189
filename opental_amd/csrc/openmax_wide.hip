// opental_amd/csrc/openmax_wide.hip -- the OpenMax layer for up to 256 classes (ActivityNet1.3: K = 150) on gfx950:
//   otal_openmax_dist_wide         : eucos distance of every feature row against the MAV of its label;
//   otal_openmax_probs_wide        : OpenMax.forward (AFSD/thumos14/openmax.py:42-86) for N rows in one launch;
//   otal_decode_clips_openmax_wide : the decode of otal_decode_clips_openmax (csrc/openmax.hip) for a batch of clips in one
//                                    launch, with the segment arithmetic of AFSD/anet/test.py:110-115.
// csrc/openmax.hip stages every class mean vector (MAV) in LDS, which ends at K = 16: at K = 150, D = 512 one stage's table is
// 300 KiB.  Here no table is staged.  openmax_recalibrate (openmax.py:42-73) gives a non-zero alpha to the R largest logits
// only (R = `rank`, 1 in the drivers); every other class has modified = logit * (1 - w * 0) = logit exactly and adds exactly 0
// to the unknown sum, so a row needs R distances, not K: O(R D + K) work per row instead of O(K D).  The R MAV rows are
// gathered from memory (both stages' tables are 600 KiB, resident in L2 after the first tiles).
//
// Layout.  A workgroup of 256 threads owns 16 feature rows, one 16-lane group per row; the rows are staged once in LDS by
// stage_feat (openmax_common.h: coalesced for the contiguous (B, A, D) layout and for the channel-major view, each element
// read once).  Class c of a row lives in slot c / 16 of lane c % 16, so a logit row is read -- and a probability row
// written -- in 64-byte runs.  Selection: R times, every lane offers its largest not-yet-taken logit and a width-16 xor
// butterfly picks the winner by (value, index); equal logits rank the HIGHER index first, as numpy's argsort()[::-1] does
// and as the narrow kernel does.  Distance: the 16 lanes walk the row and the winner's MAV as float4, 256 contiguous bytes
// per step; every lane keeps 4 partial sums (channel d goes to lane (d / 4) % 16, component d % 4: 64 partial sums of 8 terms
// at D = 512, against 16 of 32 terms in the narrow kernel) per dot product f.f, f.m, m.m and |f - m|^2, added as
// (x + y) + (z + w) and then by the xor butterfly: a fixed order that does not depend on the feature's memory layout, no
// atomics, the same bits on every lane and in every run.  The w-score is the stable fp32 form of openmax.hip's header.
// The unknown sum adds the R terms in rank order.  The softmax runs over K + 1 exponents with their maximum subtracted.
// Decode: both stages, one after the other, their average times sigmoid(center); score / flag go through an LDS
// transposition (the staged rows are dead by then) so that consecutive lanes store consecutive anchors of one class.
// Rows beyond N (beyond A in the last tile of a clip) read a clamped row and are not stored.
#include "openmax_common.h"

namespace {

constexpr int OMW_L = 16;             // lanes per row
constexpr int OMW_SLOTS = 16;         // class slots per lane
constexpr int OMW_MAXK = OMW_L * OMW_SLOTS;
constexpr int OMW_TLD = OMX_TR + 1;   // row length of the (class, anchor) transposition buffer
static_assert(OMX_THREADS == OMX_TR * OMW_L, "one 16-lane group per row");

__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
    for (int o = OMW_L / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, OMW_L);
    return v;
}

__device__ __forceinline__ float group_max(float v) {
#pragma unroll
    for (int o = OMW_L / 2; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, OMW_L));
    return v;
}

// compute_eucos_dist (openmax.py:7-9) of the LDS row `f` against the MAV row `m` in memory, by the 16 lanes of a group;
// every lane returns the same bits
__device__ __forceinline__ float group_eucos(const float* f, const float* __restrict__ m, int D, int l) {
    float ff[4] = {0.f, 0.f, 0.f, 0.f}, fm[4] = {0.f, 0.f, 0.f, 0.f}, mm[4] = {0.f, 0.f, 0.f, 0.f}, ee[4] = {0.f, 0.f, 0.f, 0.f};
    const int steps = (D + 4 * OMW_L - 1) / (4 * OMW_L);
#pragma unroll 2
    for (int t = 0; t < steps; ++t) {
        const int ch = 4 * (OMW_L * t + l);
        const bool live = ch < D;                           // D % 16 == 0: a float4 is inside the row or outside it
        const int cc = live ? ch : 0;
        float4 a = *reinterpret_cast<const float4*>(f + cc);
        float4 b = *reinterpret_cast<const float4*>(m + cc);
        if (!live) a = b = make_float4(0.f, 0.f, 0.f, 0.f);
        const float av[4] = {a.x, a.y, a.z, a.w}, bv[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            ff[i] = fmaf(av[i], av[i], ff[i]);
            fm[i] = fmaf(av[i], bv[i], fm[i]);
            mm[i] = fmaf(bv[i], bv[i], mm[i]);
            const float e = av[i] - bv[i];
            ee[i] = fmaf(e, e, ee[i]);
        }
    }
    const float sff = group_sum((ff[0] + ff[1]) + (ff[2] + ff[3]));
    const float sfm = group_sum((fm[0] + fm[1]) + (fm[2] + fm[3]));
    const float smm = group_sum((mm[0] + mm[1]) + (mm[2] + mm[3]));
    const float see = group_sum((ee[0] + ee[1]) + (ee[2] + ee[3]));
    return sqrtf(see) / 200.0f + (1.0f - sfm / (sqrtf(sff) * sqrtf(smm)));
}

// openmax_recalibrate + compute_openmax_prob (openmax.py:21-73) for one row by its 16-lane group.  In: z[s] = logit of class
// 16 s + l (anything where that class is >= K).  Out: z[s] = P(class 16 s + l); returns P(unknown), the same on every lane.
__device__ __forceinline__ float recalibrate_row(float (&z)[OMW_SLOTS], const float* f, const float* __restrict__ mav,
                                                 const float* __restrict__ wb, int K, int D, int R, int l) {
    unsigned taken = 0;                                     // bit s: class 16 s + l is out of the selection
#pragma unroll
    for (int s = 0; s < OMW_SLOTS; ++s)
        if (OMW_L * s + l >= K) taken |= 1u << s;
    float su = 0.f;
    for (int i = 0; i < R; ++i) {
        float bv = -INFINITY;
        int bc = -1;
#pragma unroll
        for (int s = 0; s < OMW_SLOTS; ++s) {               // ascending class index: >= keeps the higher index of equals
            const bool free_ = !((taken >> s) & 1u);
            if (free_ && (z[s] >= bv || bc < 0)) { bv = z[s]; bc = OMW_L * s + l; }
        }
#pragma unroll
        for (int o = OMW_L / 2; o > 0; o >>= 1) {
            const float ov = __shfl_xor(bv, o, OMW_L);
            const int oc = __shfl_xor(bc, o, OMW_L);
            const bool take = oc >= 0 && (bc < 0 || ov > bv || (ov == bv && oc > bc));
            if (take) { bv = ov; bc = oc; }
        }
        // 1 <= R <= K: there is a free class, and every lane of the group holds the same (bv, bc).  (NaN logits compare false
        // both ways and can leave the lanes in disagreement: the row is NaN then, but no address may depend on it.)
        const int cls = max(bc, 0);
        const float d = group_eucos(f, mav + (size_t)cls * D, D, l);
        const float alpha = (float)(R - i) / (float)R;
        const float mod = bv * (1.0f - w_score(d, wb + cls * 3) * alpha);
        su += bv - mod;
#pragma unroll
        for (int s = 0; s < OMW_SLOTS; ++s)
            if (OMW_L * s + l == bc) { z[s] = mod; taken |= 1u << s; }
    }
    float mx = -INFINITY;
#pragma unroll
    for (int s = 0; s < OMW_SLOTS; ++s)
        if (OMW_L * s + l < K) mx = fmaxf(mx, z[s]);
    mx = fmaxf(group_max(mx), su);
    float se = 0.f;
#pragma unroll
    for (int s = 0; s < OMW_SLOTS; ++s) {
        z[s] = OMW_L * s + l < K ? expf(z[s] - mx) : 0.f;
        se += z[s];
    }
    const float eu = expf(su - mx);
    const float den = group_sum(se) + eu;
#pragma unroll
    for (int s = 0; s < OMW_SLOTS; ++s) z[s] = z[s] / den;
    return eu / den;
}

__device__ __forceinline__ void load_logits(float (&z)[OMW_SLOTS], const float* __restrict__ row, int K, int l) {
#pragma unroll
    for (int s = 0; s < OMW_SLOTS; ++s)
        if (OMW_L * s < K) z[s] = row[min(OMW_L * s + l, K - 1)];      // a clamped class; never ranked, never stored
        else z[s] = 0.f;
}

// MODE 1: dist (N,) of each row against the MAV of its label; 2: probs (N, K + 1); 3: decode.
template <int MODE>
__global__ __launch_bounds__(OMX_THREADS) void openmax_wide_kernel(OmxArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int K = a.K, D = a.D, ld = D + OMX_PAD;
    float* sF0 = reinterpret_cast<float*>(smem);
    float* sF1 = (MODE == 3 && a.two_feats) ? sF0 + OMX_TR * ld : sF0;
    int n0, nvalid, clip, row0;
    omx_tile<MODE == 3>(a, n0, nvalid, clip, row0);
    stage_feat(sF0, ld, a.f0, n0, nvalid, D);
    if constexpr (MODE == 3)
        if (a.two_feats) stage_feat(sF1, ld, a.f1, n0, nvalid, D);
    __syncthreads();
    const int r = threadIdx.x / OMW_L, l = threadIdx.x % OMW_L;
    const bool rv = r < nvalid;
    const int rc = min(r, nvalid - 1);                      // a row past the end works on the last one and stores nothing
    const int n = n0 + rc;
    const float* f0 = sF0 + rc * ld;
    if constexpr (MODE == 1) {
        const int lab = a.labels[n];
        const bool known = lab >= 0 && lab < K;             // uniform over the group
        const float d = group_eucos(f0, a.mav0 + (size_t)(known ? lab : 0) * D, D, l);
        if (rv && l == 0) a.out[n] = known ? d : -1.0f;
    } else if constexpr (MODE == 2) {
        float z[OMW_SLOTS];
        load_logits(z, a.logit0 + (long long)n * a.ldl, K, l);
        const float pu = recalibrate_row(z, f0, a.mav0, a.wb0, K, D, a.R, l);
        if (rv) {
            float* o = a.out + (size_t)n * (K + 1);
#pragma unroll
            for (int s = 0; s < OMW_SLOTS; ++s)
                if (OMW_L * s + l < K) o[1 + OMW_L * s + l] = z[s];
            if (l == 0) o[0] = pu;
        }
    } else {
        float z0[OMW_SLOTS], z1[OMW_SLOTS];
        load_logits(z0, a.logit0 + (long long)n * a.ldl, K, l);
        load_logits(z1, a.logit1 + (long long)n * a.ldl, K, l);
        const float pu0 = recalibrate_row(z0, f0, a.mav0, a.wb0, K, D, a.R, l);
        const float pu1 = recalibrate_row(z1, sF1 + rc * ld, a.mav1, a.wb1, K, D, a.R, l);
        const float ct = omx_sigmoid(a.center[n]);
        __syncthreads();                                    // every group is done with the staged rows
        float* sT = reinterpret_cast<float*>(smem);         // (K, 17): score of class c, row r at c * 17 + r
#pragma unroll
        for (int s = 0; s < OMW_SLOTS; ++s)
            if (OMW_L * s + l < K) sT[(OMW_L * s + l) * OMW_TLD + r] = (z0[s] + z1[s]) / 2.0f * ct;
        if (rv && l == 0) {
            const int i = row0 + r;
            a.unknown[n] = (pu0 + pu1) / 2.0f * ct;
            // segments (anet/test.py:110-115)
            decode_segment(a.loc, a.prop_loc, a.priors, a.offsets, a.fps, a.seg, n, i, clip, a.clip_length);
        }
        __syncthreads();
        for (int i = threadIdx.x; i < K * OMX_TR; i += OMX_THREADS) {
            const int c = i / OMX_TR, rr = i % OMX_TR;
            if (rr < nvalid) {
                const size_t o = ((size_t)clip * K + c) * a.A + row0 + rr;
                const float sc = sT[c * OMW_TLD + rr];
                a.score[o] = sc;
                a.flag[o] = sc > a.conf_thresh;
            }
        }
    }
}

template <int MODE>
int launch_wide(const OmxArgs& a, int blocks, void* stream) {
    const size_t rows = (size_t)(1 + (MODE == 3 && a.two_feats)) * OMX_TR * (a.D + OMX_PAD) * sizeof(float);
    const size_t trans = MODE == 3 ? (size_t)a.K * OMW_TLD * sizeof(float) : 0;
    return omx_launch<openmax_wide_kernel<MODE>>(a, blocks, rows > trans ? rows : trans, stream);
}

}  // namespace

extern "C" int otal_openmax_dist_wide(const float* feat, int N, int rows_per_batch, int64_t sb, int64_t sr, int64_t sc,
                                      const float* mav, int K, int D, const int* labels, float* dist, void* stream) {
    if (!feat || !mav || !labels || !dist) return OTAL_E_NULL;
    OmxArgs a;
    if (int e = omx_rows_args(feat, N, rows_per_batch, sb, sr, sc, mav, K, D, 1, K, OMW_MAXK, a)) return e;
    a.labels = labels; a.out = dist;
    return launch_wide<1>(a, omx_tiles(N), stream);
}

extern "C" int otal_openmax_probs_wide(const float* logits, int64_t ldl, const float* feat, int N, int rows_per_batch,
                                       int64_t sb, int64_t sr, int64_t sc, const float* mav, const float* wb, int K, int D,
                                       int R, float* probs, void* stream) {
    if (!logits || !feat || !mav || !wb || !probs) return OTAL_E_NULL;
    OmxArgs a;
    if (int e = omx_rows_args(feat, N, rows_per_batch, sb, sr, sc, mav, K, D, R, ldl, OMW_MAXK, a)) return e;
    a.wb0 = wb; a.logit0 = logits; a.out = probs;
    return launch_wide<2>(a, omx_tiles(N), stream);
}

extern "C" int otal_decode_clips_openmax_wide(const float* loc, const float* prop_loc, const float* priors, const float* conf,
                                              const float* prop_conf, const float* center, const float* offsets,
                                              const float* fps, const float* feat, const float* prop_feat,
                                              const int64_t* feat_strides, const int64_t* prop_feat_strides,
                                              const float* mav, const float* mav_prop, const float* wb, const float* wb_prop,
                                              float* seg, float* score, float* unknown, unsigned char* flag, int nclips, int A,
                                              int C, int first_class, int D, int R, int refined_feature, float clip_length,
                                              float conf_thresh, void* stream) {
    OmxArgs a;
    if (int e = omx_decode_args(loc, prop_loc, priors, conf, prop_conf, center, offsets, fps, feat, prop_feat, feat_strides,
                                prop_feat_strides, mav, mav_prop, wb, wb_prop, seg, score, unknown, flag, nclips, A, C,
                                first_class, D, R, refined_feature, clip_length, conf_thresh, OMW_MAXK, a))
        return e;
    return launch_wide<3>(a, nclips * omx_tiles(A), stream);
}

