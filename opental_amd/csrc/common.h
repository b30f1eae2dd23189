// opental_amd/csrc/common.h -- shared device/host helpers for libopental_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "opental_hip.h"
#include "options.h"

#define OTAL_WAVE 64

struct LevelTab {          // passed by value as a kernel argument (lives in SGPRs)
    int nlev;
    int ts[OTAL_MAX_LEVELS + 1];   // column starts of each level along T
    int ns[OTAL_MAX_LEVELS + 1];   // column starts of each level along N (proposals)
};

typedef unsigned short bf16_t;     // raw bfloat16 bits

__device__ __forceinline__ float bf16_to_f32(bf16_t v) { return __uint_as_float(((unsigned)v) << 16); }
__device__ __forceinline__ bf16_t f32_to_bf16(float f) {          // round to nearest even
    unsigned u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (bf16_t)((u >> 16) | 0x40);   // quiet NaN
    u += 0x7fffu + ((u >> 16) & 1u);
    return (bf16_t)(u >> 16);
}
__device__ __forceinline__ float ld_f32(const float* p, size_t i) { return p[i]; }
__device__ __forceinline__ float ld_f32(const bf16_t* p, size_t i) { return bf16_to_f32(p[i]); }
__device__ __forceinline__ void st_f32(float* p, size_t i, float v) { p[i] = v; }
__device__ __forceinline__ void st_f32(bf16_t* p, size_t i, float v) { p[i] = f32_to_bf16(v); }

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// The late-fusion segment rule of every decode kernel (decode_predictions, AFSD/thumos14/test.py:114-120; anet/test.py:110-115):
// the refined offsets scale with the coarse width, the segment is clamped to the clip and leaves in seconds.  Anchor i of
// clip c is row n = c * A + i of loc, prop_loc and seg (n, 2); priors (A) are centres in [0, 1]; offsets and fps are per clip.
// The rule is stated once, on the four map values of the anchor (l0, l1 of loc, p0, p1 of prop_loc): the kernels that read them
// straight from memory use the pointer form below, the two-stream decode hands in the finished averages of two networks' maps.
__device__ __forceinline__ void decode_segment(float l0, float l1, float p0, float p1, const float* priors,
                                               const float* offsets, const float* fps, float* seg, size_t n, int i, int c,
                                               float clip_length) {
    const float w = l0 + l1;
    const float r0 = 0.5f * w * p0 + l0;
    const float r1 = 0.5f * w * p1 + l1;
    const float pc = priors[i] * clip_length;
    const float s0 = fminf(fmaxf(pc - r0, 0.f), clip_length);
    const float s1 = fminf(fmaxf(pc + r1, 0.f), clip_length);
    seg[n * 2] = (s0 + offsets[c]) / fps[c];
    seg[n * 2 + 1] = (s1 + offsets[c]) / fps[c];
}
__device__ __forceinline__ void decode_segment(const float* loc, const float* prop_loc, const float* priors,
                                               const float* offsets, const float* fps, float* seg, size_t n, int i, int c,
                                               float clip_length) {
    decode_segment(loc[n * 2], loc[n * 2 + 1], prop_loc[n * 2], prop_loc[n * 2 + 1], priors, offsets, fps, seg, n, i, c,
                   clip_length);
}

static inline int otal_launch_status() {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}
static inline int ilog2_ceil(int v) { int l = 0; while ((1 << l) < v) ++l; return l; }

// the kernel (or host-side path) that served this thread's most recent max-pool / GroupNorm / glue call, "" after a call that
// launched nothing: otal_layer_last_kernel().  Entry points clear it first and name what they launched through this helper.
extern thread_local const char* g_layer_kernel;
static inline int otal_layer_launched(const char* name) {
    const int e = otal_launch_status();
    g_layer_kernel = e == 0 ? name : "";
    return e;
}
