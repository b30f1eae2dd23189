// opental_amd/csrc/openmax_common.h -- what the OpenMax kernels of csrc/openmax.hip (K <= 16, MAVs staged in LDS) and
// csrc/openmax_wide.hip (K <= 256, MAV rows gathered) share: the strided feature view, the coalesced staging of a tile of
// 16 feature rows into LDS for either memory layout, and the stable fp32 w-score (see the header of openmax.hip).
#pragma once
#include "common.h"

namespace {

constexpr int OMX_TR = 16;            // feature rows per workgroup
constexpr int OMX_THREADS = 256;
constexpr int OMX_MAXD = 512;
constexpr int OMX_PAD = 4;            // floats of padding per LDS row

// feature rows addressed by element strides: row n, channel d at p + (n / rpb) * sb + (n % rpb) * sr + d * sc
struct FeatView { const float* p; int rpb; long long sb, sr, sc; };

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

}  // namespace
