// opental_amd/csrc/openmax_common.h -- what the OpenMax kernels of csrc/openmax.hip (K <= 16, MAVs staged in LDS) and
// csrc/openmax_wide.hip (K <= 256, MAV rows gathered) share: the strided feature view, the coalesced staging of a tile of
// 16 feature rows into LDS for either memory layout, the stable fp32 w-score (see the header of openmax.hip), the kernel
// argument record, the workgroup -> rows mapping, the launch and the entry points' argument checks.
#pragma once
#include "common.h"

namespace {

constexpr int OMX_TR = 16;            // feature rows per workgroup
constexpr int OMX_THREADS = 256;
constexpr int OMX_MAXD = 512;
constexpr int OMX_PAD = 4;            // floats of padding per LDS row

// feature rows addressed by element strides: row n, channel d at p + (n / rpb) * sb + (n % rpb) * sr + d * sc
struct FeatView { const float* p; int rpb; long long sb, sr, sc; };

struct OmxArgs {
    FeatView f0, f1;                  // coarse feature; feature of the second stage (decode; may be the same view)
    const float *mav0, *mav1;         // (K, D)
    const float *wb0, *wb1;           // (K, 3): off, inv_scale, shape
    const float *logit0, *logit1;     // row n, class j at logit[n * ldl + j]
    long long ldl;
    const int* labels;
    float* out;                       // dist (N, K) / (N,), probs (N, K + 1)
    const float *loc, *prop_loc, *priors, *center, *offsets, *fps;
    float *seg, *score, *unknown;
    unsigned char* flag;
    int N, A, K, D, R, two_feats;
    float clip_length, conf_thresh;
};

// The rows of workgroup blockIdx.x: n0 .. n0 + nvalid - 1 of the N rows, OMX_TR to a workgroup.  DECODE: a tile never
// crosses a clip -- rows row0 .. row0 + nvalid - 1 of the A anchors of `clip`.
template <bool DECODE>
__device__ __forceinline__ void omx_tile(const OmxArgs& a, int& n0, int& nvalid, int& clip, int& row0) {
    clip = row0 = 0;
    if constexpr (DECODE) {
        const int tiles = (a.A + OMX_TR - 1) / OMX_TR;
        clip = blockIdx.x / tiles;
        row0 = (blockIdx.x - clip * tiles) * OMX_TR;
        n0 = clip * a.A + row0;
        nvalid = min(OMX_TR, a.A - row0);
    } else {
        n0 = blockIdx.x * OMX_TR;
        nvalid = min(OMX_TR, a.N - n0);
    }
}

__device__ __forceinline__ const float* feat_row(const FeatView& f, int n) {
    return f.p + (long long)(n / f.rpb) * f.sb + (long long)(n % f.rpb) * f.sr;
}

__device__ __forceinline__ float omx_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

__device__ __forceinline__ bool aligned16(const FeatView& f) {
    return f.sc == 1 && ((uintptr_t)f.p & 15) == 0 && (f.sb & 3) == 0 && (f.sr & 3) == 0;
}

// rows n0 .. n0 + OMX_TR - 1 (the first `nvalid` exist, the rest are zero-filled) -> s[r * ld + d]
__device__ void stage_feat(float* s, int ld, const FeatView& f, int n0, int nvalid, int D) {
    const int t = threadIdx.x;
    if (aligned16(f)) {
        const int q4 = D >> 2, total = OMX_TR * q4;
#pragma unroll 4
        for (int i = t; i < total; i += OMX_THREADS) {
            const int r = i / q4, q = i - r * q4;
            // unconditional load from a clamped row, then select: a guarded load becomes a branch with a full wait behind it
            float4 v = *reinterpret_cast<const float4*>(feat_row(f, n0 + min(r, nvalid - 1)) + 4 * q);
            if (r >= nvalid) v = make_float4(0.f, 0.f, 0.f, 0.f);
            *reinterpret_cast<float4*>(s + r * ld + 4 * q) = v;
        }
    } else {
        const int total = OMX_TR * D;
        const bool rows_fastest = (f.sr < 0 ? -f.sr : f.sr) < (f.sc < 0 ? -f.sc : f.sc);
#pragma unroll 8
        for (int i = t; i < total; i += OMX_THREADS) {
            const int r = rows_fastest ? i % OMX_TR : i / D;
            const int d = rows_fastest ? i / OMX_TR : i - (i / D) * D;
            const float v = feat_row(f, n0 + min(r, nvalid - 1))[(long long)d * f.sc];
            s[r * ld + d] = r < nvalid ? v : 0.f;
        }
    }
}

// w_score of libMR (MetaRecognition.cpp:141-152 -> weibull_cdf) in the stable fp32 form of the header of openmax.hip
__device__ __forceinline__ float w_score(float d, const float* wb) {
    const float u = (d - wb[0]) * wb[1];
    if (u <= -1.0f) return 0.f;
    return -expm1f(-expf(wb[2] * log1pf(u)));
}

// `blocks` workgroups of KERNEL with `lds` bytes of dynamic LDS (beyond 48 KiB the limit has to be raised first)
template <void (*KERNEL)(OmxArgs)>
int omx_launch(const OmxArgs& a, int blocks, size_t lds, void* stream) {
    if (lds > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(KERNEL, dim3(blocks), dim3(OMX_THREADS), lds, (hipStream_t)stream, a);
    return otal_launch_status();
}

inline int omx_tiles(int rows) { return (rows + OMX_TR - 1) / OMX_TR; }

// The entry points' checks come in the order NULL (theirs), SHAPE, UNSUPPORTED and precede every launch.
inline int omx_check_dims(int N, int rpb, int K, int D, int R, int max_k) {
    if (N <= 0 || rpb <= 0 || K <= 0 || D <= 0) return OTAL_E_SHAPE;
    if (K > max_k || D > OMX_MAXD || (D & 15) || R < 1 || R > K) return OTAL_E_UNSUPPORTED;
    return 0;
}

// dist / probs: N feature rows against one (K, D) MAV table; logit rows of length ldl (dist: pass K)
inline int omx_rows_args(const float* feat, int N, int rpb, int64_t sb, int64_t sr, int64_t sc, const float* mav, int K, int D,
                         int R, int64_t ldl, int max_k, OmxArgs& a) {
    if (ldl < K) return OTAL_E_SHAPE;
    if (int e = omx_check_dims(N, rpb, K, D, R, max_k)) return e;
    if ((uintptr_t)mav & 15) return OTAL_E_UNSUPPORTED;
    a = {};
    a.f0 = a.f1 = FeatView{feat, rpb, (long long)sb, (long long)sr, (long long)sc};
    a.mav0 = mav; a.ldl = ldl; a.N = N; a.K = K; a.D = D; a.R = R;
    return 0;
}

// the decode entries (same arguments in both kernel families): every check, then the kernel arguments
inline int omx_decode_args(const float* loc, const float* prop_loc, const float* priors, const float* conf,
                           const float* prop_conf, const float* center, const float* offsets, const float* fps,
                           const float* feat, const float* prop_feat, const int64_t* feat_strides,
                           const int64_t* prop_feat_strides, const float* mav, const float* mav_prop, const float* wb,
                           const float* wb_prop, float* seg, float* score, float* unknown, unsigned char* flag, int nclips, int A,
                           int C, int first_class, int D, int R, int refined_feature, float clip_length, float conf_thresh,
                           int max_k, OmxArgs& a) {
    if (!loc || !prop_loc || !priors || !conf || !prop_conf || !center || !offsets || !fps || !feat || !feat_strides ||
        !mav || !mav_prop || !wb || !wb_prop || !seg || !score || !unknown || !flag)
        return OTAL_E_NULL;
    if (refined_feature && (!prop_feat || !prop_feat_strides)) return OTAL_E_NULL;
    if (nclips <= 0 || A <= 0 || C <= 0 || first_class < 0 || C - first_class <= 0) return OTAL_E_SHAPE;
    if ((long long)nclips * A > 0x7fffffffLL) return OTAL_E_SHAPE;
    const int K = C - first_class;
    if (int e = omx_check_dims(nclips * A, A, K, D, R, max_k)) return e;
    if (refined_feature < 0 || refined_feature > 1 || ((uintptr_t)mav & 15) || ((uintptr_t)mav_prop & 15))
        return OTAL_E_UNSUPPORTED;
    a = {};
    a.f0 = FeatView{feat, A, (long long)feat_strides[0], (long long)feat_strides[1], (long long)feat_strides[2]};
    a.f1 = refined_feature ? FeatView{prop_feat, A, (long long)prop_feat_strides[0], (long long)prop_feat_strides[1],
                                      (long long)prop_feat_strides[2]}
                           : a.f0;
    a.two_feats = refined_feature;
    a.mav0 = mav; a.mav1 = mav_prop; a.wb0 = wb; a.wb1 = wb_prop;
    a.logit0 = conf + first_class; a.logit1 = prop_conf + first_class; a.ldl = C;
    a.loc = loc; a.prop_loc = prop_loc; a.priors = priors; a.center = center; a.offsets = offsets; a.fps = fps;
    a.seg = seg; a.score = score; a.unknown = unknown; a.flag = flag;
    a.N = nclips * A; a.A = A; a.K = K; a.D = D; a.R = R; a.clip_length = clip_length; a.conf_thresh = conf_thresh;
    return 0;
}

}  // namespace
