// opental_amd/csrc/common.h -- shared device/host helpers for libopental_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "opental_hip.h"

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

static inline int otal_launch_status() {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}
static inline int ilog2_ceil(int v) { int l = 0; while ((1 << l) < v) ++l; return l; }

// Named run-time switches: the kernel-selection references the tests flip (otal_set_option).  The table is the only place
// a switch is named with its default; OTAL_OPT("NAME") of a name not in it does not compile.
struct OtalOption { const char* name; int dflt; };
constexpr OtalOption OTAL_OPTIONS[] = {
    {"OTAL_CONV_1A_NOTILE", 0},           {"OTAL_CONV_1A_WGS", 0},      // 0: one workgroup per compute unit
    {"OTAL_CONV_DIRECT_MINTILES", 140},   {"OTAL_CONV_DIRECT_MINTILES512", 512},
    {"OTAL_CONV_DIRECT_XPF2", 3},         {"OTAL_CONV_NO1A", 0},
    {"OTAL_CONV_NO1AW", 0},               {"OTAL_CONV_NO1DTILE", 0},
    {"OTAL_CONV_NO1X1STREAM", 0},         {"OTAL_CONV_NODIRECT", 0},
    {"OTAL_CONV_NOPROJ", 0},              {"OTAL_CONV_NOPROJW", 0},
    {"OTAL_CONV_NOW1D", 0},               {"OTAL_CONV_NOW1X1", 0},
    {"OTAL_CONV_NOWDIRECT", 0},           {"OTAL_LOSS_NOSTAGE", 0},
    {"OTAL_POOL_NO133", 0},               {"OTAL_POOL_NOROWS", 0},
    {"OTAL_W1A_SPLITS", 0},               {"OTAL_WDIRECT_BLOCKS", 0},   // 0: the launcher's own choice
};
constexpr int OTAL_NUM_OPTIONS = sizeof(OTAL_OPTIONS) / sizeof(OTAL_OPTIONS[0]);
constexpr bool otal_streq(const char* a, const char* b) { return *a == *b && (*a == 0 || otal_streq(a + 1, b + 1)); }
constexpr int otal_option_index(const char* name, int i = 0) {
    return i == OTAL_NUM_OPTIONS ? -1 : otal_streq(OTAL_OPTIONS[i].name, name) ? i : otal_option_index(name, i + 1);
}
// The value of switch `index` (core.hip): its first lookup reads the environment variable of the same name (absent: the
// default; present but not a number: 1), later lookups are one load.  Never getenv() on a launch path.
int* otal_option_slot(int index);
#define OTAL_OPT(name) ([]() -> int {                                                                              \
    constexpr int index_ = otal_option_index(name);                                                              \
    static_assert(index_ >= 0, "unknown option " name " (common.h: OTAL_OPTIONS)");                               \
    static int* const slot_ = otal_option_slot(index_);                                                          \
    return *slot_;                                                                                               \
}())
