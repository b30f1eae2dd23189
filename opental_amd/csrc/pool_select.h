// opental_amd/csrc/pool_select.h -- which kernel serves a max-pool launch: the geometry, every predicate the choice reads, the
// launch sizes it implies, and pool_choose(), the one place the order of the kernels is written down.  Shared by pool3d.hip
// (the kernels and their launches) and a plain-C++ CPU harness (tests/cpu_pool_select.cpp) that pins the choice for every
// pool call the tests make.  No HIP types in here.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/opental_hip.h"
#include "conv_index.h"
#include "options.h"

namespace {

struct PoolGeom {          // also a by-value kernel argument: its layout is part of every pool kernel
    int B, C, Ti, Hi, Wi, To, Ho, Wo;
    int kt, kh, kw, st, sh, sw, pt, ph, pw;
    int64_t x_bs, x_cs, y_bs, y_cs;
    FastDiv fWo, fHo, fWi, fHi;
    // LDS-staged kernels
    int HL, WL;            // forward: staged input plane incl. halo  ((Ho-1)*sh + kh, (Wo-1)*sw + kw)
    int HLo, WLo, ho_min, wo_min;   // backward: staged dy/arg plane incl. halo, first staged ho / wo (<= 0)
    FastDiv fPo, fPi, fPL, fWL, fPLo, fWLo;   // Ho*Wo, Hi*Wi, HL*WL, WL, HLo*WLo, WLo
};

static inline int fill(PoolGeom& g, const int* d, const int64_t* s) {
    // d: B,C, Ti,Hi,Wi, To,Ho,Wo, kt,kh,kw, st,sh,sw, pt,ph,pw
    g.B = d[0]; g.C = d[1]; g.Ti = d[2]; g.Hi = d[3]; g.Wi = d[4]; g.To = d[5]; g.Ho = d[6]; g.Wo = d[7];
    g.kt = d[8]; g.kh = d[9]; g.kw = d[10]; g.st = d[11]; g.sh = d[12]; g.sw = d[13];
    g.pt = d[14]; g.ph = d[15]; g.pw = d[16];
    for (int i = 0; i < 14; ++i) if (d[i] <= 0) return OTAL_E_SHAPE;
    if (g.kt * g.kh * g.kw > 254) return OTAL_E_UNSUPPORTED;
    if ((int64_t)g.B * g.C > 65535) return OTAL_E_UNSUPPORTED;
    if ((int64_t)g.Ti * g.Hi * g.Wi >= (1LL << 31)) return OTAL_E_SHAPE;
    g.x_bs = s[0]; g.x_cs = s[1]; g.y_bs = s[2]; g.y_cs = s[3];
    g.fWo = make_fastdiv(g.Wo); g.fHo = make_fastdiv(g.Ho); g.fWi = make_fastdiv(g.Wi); g.fHi = make_fastdiv(g.Hi);
    g.HL = (g.Ho - 1) * g.sh + g.kh; g.WL = (g.Wo - 1) * g.sw + g.kw;
    const int ch = (g.kh + g.sh - 1) / g.sh, cw = (g.kw + g.sw - 1) / g.sw;
    g.ho_min = -(ch - 1); g.wo_min = -(cw - 1);
    g.HLo = (g.Hi - 1 + g.ph) / g.sh - g.ho_min + 1; g.WLo = (g.Wi - 1 + g.pw) / g.sw - g.wo_min + 1;
    g.fPo = make_fastdiv((uint32_t)(g.Ho * g.Wo)); g.fPi = make_fastdiv((uint32_t)(g.Hi * g.Wi));
    g.fPL = make_fastdiv((uint32_t)(g.HL * g.WL)); g.fWL = make_fastdiv((uint32_t)g.WL);
    g.fPLo = make_fastdiv((uint32_t)(g.HLo * g.WLo)); g.fWLo = make_fastdiv((uint32_t)g.WLo);
    return 0;
}

constexpr size_t POOL_LDS_BUDGET = 48 * 1024;
// output planes per block (forward): ~4096 outputs, staged input planes within the LDS budget; 0 = does not fit
static inline int fwd_planes(const PoolGeom& g, size_t& lds) {
    int tt = 4096 / (g.Ho * g.Wo);
    if (tt < 1) tt = 1;
    if (tt > g.To) tt = g.To;
    for (; tt >= 1; --tt) {
        lds = (size_t)((tt - 1) * g.st + g.kt) * g.HL * g.WL * sizeof(float);
        if (lds <= POOL_LDS_BUDGET) return tt;
    }
    return 0;
}
// input planes per block (backward) + the largest number of output planes a block stages
static inline int bwd_planes(const PoolGeom& g, int& tlo_max, size_t& lds) {
    int ti = 4096 / (g.Hi * g.Wi);
    if (ti < 1) ti = 1;
    if (ti > g.Ti) ti = g.Ti;
    const int ct = (g.kt + g.st - 1) / g.st;
    for (; ti >= 1; --ti) {
        tlo_max = (ti - 1 + g.st - 1) / g.st + ct + 1;      // >= toB - toA + 1 for every tile origin
        lds = (size_t)tlo_max * g.HLo * g.WLo * (sizeof(float) + 1) + 16;
        if (lds <= POOL_LDS_BUDGET) return ti;
    }
    return 0;
}

// ---- the shapes with kernels of their own
// The strided 3x3 pools -- 1: (1,3,3)/(1,2,2), 3: (3,3,3)/(2,2,2), 0: neither (or OTAL_POOL_NO133).  Geometry and strides
// only: this is also what decides whether a pool can keep its ReLU mask as sign bits (otal_maxpool3d_signbits_bytes).
static inline int strided_k33_kind(const PoolGeom& g) {
    if (!(g.kh == 3 && g.kw == 3 && g.sh == 2 && g.sw == 2 && g.pt == 0 && g.ph == 0 && g.pw == 0 && g.Hi % 2 == 0 && g.Wi % 4 == 0 &&
          g.Ho == g.Hi / 2 && g.Wo == g.Wi / 2 && g.x_bs % 4 == 0 && g.x_cs % 4 == 0 && g.y_bs % 2 == 0 && g.y_cs % 2 == 0)) return 0;
    if (OTAL_OPT("OTAL_POOL_NO133")) return 0;
    if (g.kt == 1 && g.st == 1 && g.To == g.Ti) return 1;
    if (g.kt == 3 && g.st == 2 && g.Ti % 2 == 0 && g.To == g.Ti / 2) return 3;
    return 0;
}
static inline bool strided_k33_aligned(uintptr_t x, uintptr_t y) { return (x & 15) == 0 && (y & 7) == 0; }      // their kernels' 16-byte x / dx, 8-byte y / dy pieces
// the Inception branch pools: 3x3x3, stride 1, pad 1, square planes of side 12 / 6 / 3 with T unchanged
static inline bool is_333_s1(const PoolGeom& g) {
    return g.kt == 3 && g.kh == 3 && g.kw == 3 && g.st == 1 && g.sh == 1 && g.sw == 1 && g.pt == 1 && g.ph == 1 && g.pw == 1 &&
           g.Hi == g.Wi && (g.Hi == 12 || g.Hi == 6 || g.Hi == 3) && g.To == g.Ti && g.Ho == g.Hi && g.Wo == g.Wi &&
           (int64_t)g.Ti * g.Hi * g.Wi < (1LL << 30);
}
static inline bool strides_multiple_of(const PoolGeom& g, int xm, int ym) { return g.x_bs % xm == 0 && g.x_cs % xm == 0 && g.y_bs % ym == 0 && g.y_cs % ym == 0; }
// ---- tiles and LDS layouts of the branch-pool kernels (the `sm` carving of each kernel, in its own order)
constexpr int POOL_SEP_ELEMS = 1152;     // plane elements per cell-per-thread workgroup (8 planes of 12x12, 32 of 6x6, 128 of 3x3)
// maxpool333_sep_fwd_kernel<P> at tt output planes: [tt+2][Q][Q] + [tt+2][Q][P] floats, [tt+2][Q][P] + [tt+2][P][P] tap bytes
static inline size_t sep_fwd_lds(int P, int tt) {
    const int Q = P + 2;
    return (size_t)(tt + 2) * (Q * Q + Q * P) * sizeof(float) + (size_t)(tt + 2) * (Q * P + P * P);
}
// maxpool333_sep_bwd_kernel<P>: [ti+2] planes of dy, 2 x [ti] planes of stage gradients, [ti+2] planes of tap bytes
static inline size_t sep_bwd_lds(int P, int ti) { return (size_t)((ti + 2) + 2 * ti) * P * P * sizeof(float) + (size_t)(ti + 2) * P * P; }
// the row-per-thread kernels: one row per thread of a 256-thread workgroup, a halo plane on each side
static inline int rows_planes(int P) { return 256 / P - 2; }
// maxpool333_rows_fwd_kernel<P>: row maxima + plane maxima; _bwd: dy + plane-stage gradients, then tap rows of pitch 12 / 8
static inline size_t rows_lds(int P, bool bwd) {
    const int rows = (rows_planes(P) + 2) * P;
    return (size_t)2 * rows * P * sizeof(float) + (bwd ? (size_t)rows * (P == 12 ? 12 : 8) : 0);
}

// ---- the choice: one value per instantiation that can run, in the order of pool_kernel_name()'s table
enum PoolKernel {
    PK_W8_NN_FWD, PK_W8_FWD, PK_K33_FWD_1HH, PK_K33_FWD_3HH, PK_K33_FWD_1HF, PK_K33_FWD_1FF, PK_K33_FWD_3FF, PK_ROWS_FWD_12H,
    PK_ROWS_FWD_6H, PK_ROWS_FWD_12, PK_ROWS_FWD_6, PK_SEP_FWD_12, PK_SEP_FWD_6, PK_SEP_FWD_3, PK_FWD_133, PK_FWD_333S1,
    PK_FWD_333S2, PK_FWD_222, PK_FWD_ANY, PK_FWD_LDS_333S1, PK_FWD_LDS_ANY,
    PK_W8_BWD, PK_K33_BWD_1HH, PK_W12_BWD, PK_K33_BWD_3HH, PK_K33_BWD_1HF, PK_K33_BWD_1FF, PK_K33_BWD_3FF, PK_ROWS_BWD_12H,
    PK_ROWS_BWD_6H, PK_ROWS_BWD_12, PK_ROWS_BWD_6, PK_SEP_BWD_12V4, PK_SEP_BWD_6V4, PK_SEP_BWD_12, PK_SEP_BWD_6, PK_SEP_BWD_3,
    PK_BWD_133, PK_BWD_333S1, PK_BWD_333S2, PK_BWD_222, PK_BWD_ANY,                     // + pool_shape_index()
    PK_BWD_LDS_133, PK_BWD_LDS_333S1, PK_BWD_LDS_333S2, PK_BWD_LDS_222, PK_BWD_LDS_ANY, PK_COUNT
};
// the kernel's name as otal_layer_last_kernel() and the tests spell it
static inline const char* pool_kernel_name(int kernel) {
    static const char* const names[PK_COUNT] = {
        "maxpool133_s2_w8_nn_fwd", "maxpool133_s2_w8_fwd", "maxpoolk33_s2_fwd<1,bf16,bf16>", "maxpoolk33_s2_fwd<3,bf16,bf16>",
        "maxpoolk33_s2_fwd<1,bf16,f32>", "maxpoolk33_s2_fwd<1,f32,f32>", "maxpoolk33_s2_fwd<3,f32,f32>", "maxpool333_rows_fwd<12,bf16>",
        "maxpool333_rows_fwd<6,bf16>", "maxpool333_rows_fwd<12,f32>", "maxpool333_rows_fwd<6,f32>", "maxpool333_sep_fwd<12>",
        "maxpool333_sep_fwd<6>", "maxpool333_sep_fwd<3>",
        "maxpool3d_fwd<133/122>", "maxpool3d_fwd<333/111>", "maxpool3d_fwd<333/222>", "maxpool3d_fwd<222/222>", "maxpool3d_fwd<generic>",
        "maxpool3d_fwd_lds<333/111>", "maxpool3d_fwd_lds<generic>",
        "maxpool133_s2_w8_bwd", "maxpoolk33_s2_bwd<1,bf16,bf16>", "maxpool333_s2_w12_bwd", "maxpoolk33_s2_bwd<3,bf16,bf16>",
        "maxpoolk33_s2_bwd<1,bf16,f32>", "maxpoolk33_s2_bwd<1,f32,f32>", "maxpoolk33_s2_bwd<3,f32,f32>", "maxpool333_rows_bwd<12,bf16>",
        "maxpool333_rows_bwd<6,bf16>", "maxpool333_rows_bwd<12,f32>", "maxpool333_rows_bwd<6,f32>",
        "maxpool333_sep_bwd<12,v4>", "maxpool333_sep_bwd<6,v4>", "maxpool333_sep_bwd<12>", "maxpool333_sep_bwd<6>", "maxpool333_sep_bwd<3>",
        "maxpool3d_bwd<133/122>", "maxpool3d_bwd<333/111>", "maxpool3d_bwd<333/222>", "maxpool3d_bwd<222/222>", "maxpool3d_bwd<generic>",
        "maxpool3d_bwd_lds<133/122>", "maxpool3d_bwd_lds<333/111>", "maxpool3d_bwd_lds<333/222>", "maxpool3d_bwd_lds<222/222>", "maxpool3d_bwd_lds<generic>"};
    return kernel >= 0 && kernel < PK_COUNT ? names[kernel] : "?";
}
// the compile-time shape of the per-element and LDS-staged kernels: 0 <133/122>, 1 <333/111>, 2 <333/222>, 3 <222/222>, 4 run-time
static inline int pool_shape_index(const PoolGeom& g) {
    const int kk = g.kt * 100 + g.kh * 10 + g.kw, ss = g.st * 100 + g.sh * 10 + g.sw;
    return kk == 133 && ss == 122 ? 0 : kk == 333 && ss == 111 ? 1 : kk == 333 && ss == 222 ? 2 : kk == 222 && ss == 222 ? 3 : 4;
}

enum { POOL_FWD = 0, POOL_BWD = 1 };
// One launch as the entry points see it.  Addresses are only tested for alignment; an absent operand has address 0.
struct PoolQuery {
    int dir, geom_rc;       // POOL_FWD / POOL_BWD; what fill() answered for g (non-zero: g is not to be read)
    PoolGeom g;
    int io;                 // as received: bf16-STORED tensors.  fwd: bit 0 x, bit 1 y (bit 2: nonneg); bwd: bit 0 dx, bit 1 dy, bit 2 out_mask
    int nonneg;             // fwd: the caller guarantees x >= +0 (a conv + ReLU output): ordered-key kernels
    int accumulate, has_mask, has_scale, has_signbits;      // (accumulate, mask, scale: bwd)
    uintptr_t x, y, argtap, signbits, mask;                 // x: fwd x, bwd dx; y: fwd y, bwd dy
};
struct PoolChoice {
    int rc;                 // 0, or the OTAL_E_* code the entry point returns (then nothing below is meaningful)
    int kernel, gx, gy;     // PoolKernel; the grid (the block is 256 threads everywhere)
    size_t lds;             // dynamic LDS bytes
    int planes, tlo_max, vec;       // planes per block (staged / branch-pool kernels); bwd_lds: output planes staged at most; sep_fwd: aligned x
};
static inline PoolChoice pool_choice(const PoolGeom& g, int kernel, int gx, size_t lds = 0, int planes = 0, int tlo_max = 0, int vec = 0) {
    return PoolChoice{0, kernel, gx, g.B * g.C, lds, planes, tlo_max, vec};      // grid y: one (sample, channel) slab
}
static inline PoolChoice pool_refusal(int rc) { return PoolChoice{rc, -1, 0, 0, 0, 0, 0, 0}; }
static inline int ceil_div(int a, int b) { return (a + b - 1) / b; }
// eight input columns per thread of a bf16 (1,3,3)/(1,2,2) pool, both directions
static inline bool w8_eligible(const PoolQuery& q) { return q.g.Wi % 8 == 0 && strides_multiple_of(q.g, 8, 4) && (q.argtap & 3) == 0 && (q.signbits & 1) == 0; }

static inline PoolChoice pool_choose_fwd(const PoolQuery& q) {
    const PoolGeom& g = q.g;
    const int io = q.io & 3;
    if (io != 0 && io != 1 && io != 3) return pool_refusal(OTAL_E_UNSUPPORTED);
    if (q.geom_rc) return pool_refusal(q.geom_rc);
    const int kind = strided_k33_aligned(q.x, q.y) ? strided_k33_kind(g) : 0;
    if ((q.has_signbits || io == 1) && !kind) return pool_refusal(OTAL_E_UNSUPPORTED);
    if (kind) {
        const int gx = ceil_div(g.To * g.Ho * (g.Wo / 2), 256);
        if (io == 3 && kind == 1 && w8_eligible(q)) return pool_choice(g, q.nonneg ? PK_W8_NN_FWD : PK_W8_FWD, ceil_div(g.To * g.Ho * (g.Wo / 4), 256));
        if (io == 3) return pool_choice(g, kind == 1 ? PK_K33_FWD_1HH : PK_K33_FWD_3HH, gx);      // bf16 in, bf16 out
        // bf16-stored input (8-byte rows), fp32 output: the (1,3,3)/(1,2,2) pools
        if (io == 1) return kind == 1 ? pool_choice(g, PK_K33_FWD_1HF, gx) : pool_refusal(OTAL_E_UNSUPPORTED);
        return pool_choice(g, kind == 1 ? PK_K33_FWD_1FF : PK_K33_FWD_3FF, gx);
    }
    if (is_333_s1(g)) {
        const int P = g.Hi, TT = rows_planes(P);
        const int vec = (strides_multiple_of(g, 4, 1) && (q.x & 15) == 0) ? 1 : 0;
        const bool rows = P == 12 || P == 6, vy = strides_multiple_of(g, 1, 4) && (q.y & 15) == 0 && (q.argtap & 3) == 0;
        if (io == 3) {          // bf16 in / out: the row-per-thread kernels (12 x 12, 6 x 6 planes; 16-byte aligned channel planes)
            if (!(rows && strides_multiple_of(g, 8, 8) && ((q.x | q.y) & 15) == 0 && (q.argtap & 3) == 0)) return pool_refusal(OTAL_E_UNSUPPORTED);
            return pool_choice(g, P == 12 ? PK_ROWS_FWD_12H : PK_ROWS_FWD_6H, ceil_div(g.To, TT), rows_lds(P, false), TT);
        }
        if (vec && vy && rows && !OTAL_OPT("OTAL_POOL_NOROWS"))      // one row per thread
            return pool_choice(g, P == 12 ? PK_ROWS_FWD_12 : PK_ROWS_FWD_6, ceil_div(g.To, TT), rows_lds(P, false), TT);
        int tt = POOL_SEP_ELEMS / (P * P) > g.To ? g.To : POOL_SEP_ELEMS / (P * P);      // (>= 1: P <= 12, To >= 1)
        while (tt > 1 && sep_fwd_lds(P, tt) > POOL_LDS_BUDGET) --tt;
        return pool_choice(g, P == 12 ? PK_SEP_FWD_12 : P == 6 ? PK_SEP_FWD_6 : PK_SEP_FWD_3, ceil_div(g.To, tt), sep_fwd_lds(P, tt), tt, 0, vec);
    }
    if (io) return pool_refusal(OTAL_E_UNSUPPORTED);      // bf16 tensors: the strided 3x3 pools and the 12 x 12 / 6 x 6 branch pools only
    // staging pays when the taps overlap (stride 1: every input is read kvol times); the strided pools read each input
    // ~2 times and were measured faster with direct loads (r01: 230 vs 514 us for the 1x3x3 / (1,2,2) pool)
    size_t lds = 0;
    const bool overlap = g.st == 1 && g.sh == 1 && g.sw == 1;
    const int tt = overlap ? fwd_planes(g, lds) : 0, shape = pool_shape_index(g);
    if (tt > 0) return pool_choice(g, shape == 1 ? PK_FWD_LDS_333S1 : PK_FWD_LDS_ANY, ceil_div(g.To, tt), lds, tt);
    return pool_choice(g, PK_FWD_133 + shape, ceil_div(g.To * g.Ho * g.Wo, 256));
}

static inline PoolChoice pool_choose_bwd(const PoolQuery& q) {
    const PoolGeom& g = q.g;
    const int io = q.io;
    if ((!q.has_mask && !q.has_signbits) != !q.has_scale || (q.has_mask && q.has_signbits)) return pool_refusal(OTAL_E_NULL);   // a scale with exactly one mask form
    const bool all_half = (io & 3) == 3 && (!q.has_mask || (io & 4));
    if (io != 0 && io != 1 && !all_half) return pool_refusal(OTAL_E_UNSUPPORTED);
    if (q.geom_rc) return pool_refusal(q.geom_rc);
    const int kind = (q.mask & 15) == 0 && strided_k33_aligned(q.x, q.y) ? strided_k33_kind(g) : 0;
    if ((q.has_signbits || io == 1) && !kind) return pool_refusal(OTAL_E_UNSUPPORTED);
    if (io == 1 && kind != 1) return pool_refusal(OTAL_E_UNSUPPORTED);
    if (io && kind && (q.accumulate || q.has_mask)) return pool_refusal(OTAL_E_UNSUPPORTED);    // bf16-stored dx of a strided pool: plain store, sign-bit mask
    if (kind) {
        const int gx = ceil_div(g.Ti * (g.Hi / 2) * (g.Wi / 4), 256);
        if (all_half && kind == 1 && w8_eligible(q)) return pool_choice(g, PK_W8_BWD, ceil_div(g.Ti * (g.Hi / 2) * (g.Wi / 8), 256));
        if (all_half && kind == 1) return pool_choice(g, PK_K33_BWD_1HH, gx);
        if (all_half && g.Wi == 12) return pool_choice(g, PK_W12_BWD, ceil_div(g.To * (g.Hi / 2), 256));   // (its stride needs are the kind's own)
        if (all_half) return pool_choice(g, PK_K33_BWD_3HH, gx);
        if (io == 1) return pool_choice(g, PK_K33_BWD_1HF, gx);
        return pool_choice(g, kind == 1 ? PK_K33_BWD_1FF : PK_K33_BWD_3FF, gx);
    }
    if (is_333_s1(g)) {
        const int P = g.Hi, TI = rows_planes(P), ti = POOL_SEP_ELEMS / (P * P);
        const bool rows = P == 12 || P == 6, a16 = ((q.y | q.x | q.mask | q.argtap) & 15) == 0;
        const bool v2 = strides_multiple_of(g, 4, 4) && a16;
        const bool v4 = v2 && ((int64_t)g.To * P * P) % 4 == 0;
        if (io) {               // bf16 dy / dx / mask: the row-per-thread kernels (12 x 12, 6 x 6 planes; 16-byte aligned channel planes)
            if (!(all_half && rows && strides_multiple_of(g, 8, 8) && a16)) return pool_refusal(OTAL_E_UNSUPPORTED);
            return pool_choice(g, P == 12 ? PK_ROWS_BWD_12H : PK_ROWS_BWD_6H, ceil_div(g.Ti, TI), rows_lds(P, true), TI);
        }
        if (v2 && rows && !OTAL_OPT("OTAL_POOL_NOROWS"))      // one input row per thread
            return pool_choice(g, P == 12 ? PK_ROWS_BWD_12 : PK_ROWS_BWD_6, ceil_div(g.Ti, TI), rows_lds(P, true), TI);
        const int kernel = P == 12 ? (v4 ? PK_SEP_BWD_12V4 : PK_SEP_BWD_12) : P == 6 ? (v4 ? PK_SEP_BWD_6V4 : PK_SEP_BWD_6) : PK_SEP_BWD_3;
        return pool_choice(g, kernel, ceil_div(g.Ti, ti), sep_bwd_lds(P, ti), ti);
    }
    if (io) return pool_refusal(OTAL_E_UNSUPPORTED);
    size_t lds = 0; int tlo_max = 0;
    const int ti = bwd_planes(g, tlo_max, lds), shape = pool_shape_index(g);
    if (ti > 0) return pool_choice(g, PK_BWD_LDS_133 + shape, ceil_div(g.Ti, ti), lds, ti, tlo_max);
    return pool_choice(g, PK_BWD_133 + shape, ceil_div(g.Ti * g.Hi * g.Wi, 256));
}
// The kernel that serves a launch, its grid, LDS size and tile arguments, or the code the entry point refuses it with.
static inline PoolChoice pool_choose(const PoolQuery& q) { return q.dir == POOL_FWD ? pool_choose_fwd(q) : pool_choose_bwd(q); }

}  // namespace
