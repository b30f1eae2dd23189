// opental_amd/csrc/conv_select.h -- which kernel serves a convolution launch: every predicate the choice reads, the sizes of
// the tables and weight packs it implies, conv_plan(), the one place the order of the kernels is written down, and
// conv_launch_shape(): the tiles, grid, split-K and cut of the workspace of one step, which the launchers of conv_gemm.hip
// and its .inc files take from here (conv1x1_stream.inc and conv1a_tile.hip shape their own launches).
// Shared by conv_gemm.hip (the launches, the prologue, storage and workspace queries), conv1a_tile.hip, and a plain-C++ CPU
// harness (tests/cpu_conv_select.cpp) that pins choice and shape per layer of the model.  No HIP types in here.
#pragma once
#include <initializer_list>
#include <stddef.h>
#include <stdint.h>
#include "conv_index.h"
#include "options.h"

namespace {

enum { MODE_FWD = 0, MODE_DGRAD = 1, MODE_WGRAD = 2 };

// tile constants the predicates read; the kernels take them from here
constexpr int C1_TT = 2, C1_TR = 2, C1_WO = 48;     // Conv3d_1a direct kernel: output planes x rows x columns per tile
constexpr int C1T_TT = 4, C1T_TR = 4;               // Conv3d_1a tiled kernel (conv1a_tile.hip): output planes x rows per tile
constexpr int C1_STEPS = 49;                        // Conv3d_1a, both kernels: (dt, dh) K steps of 64 bytes per packed weight row
constexpr int W1_TC = 128;                          // 1-D weight gradient: positions per chunk
constexpr int PJ_HW = 36;                           // projection forward: the 6 x 6 plane the kernel collapses
constexpr int PW_KS = 32;                           // projection weight gradient: frames per K step
constexpr size_t TAB_PAD = 64;      // generic tap table: entries readable past K (a K step may run up to BK-1 rows over)
constexpr int CHUNK_PAD = 16;       // chunk table: entries readable past Kp/8 (two K steps of prefetch)
constexpr int PTAB_PAD = 64;        // position table: entries readable past the last group (two K steps of prefetch at CW = 2 -> 32)

// ---- sizes of tables and weight packs (the tables hold int2 entries)
static inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }
static inline size_t tab_bytes(int K) { return (((size_t)K + TAB_PAD) * (2 * sizeof(int)) + 255) & ~(size_t)255; }
static inline int chunk_kp(int K) { return (K + 31) / 32 * 32; }
static inline size_t chunk_tab_bytes(int K) { return align256(((size_t)chunk_kp(K) / 8 + CHUNK_PAD) * (2 * sizeof(int))); }
static inline size_t chunk_wp_bytes(int M, int BM, int K) {      // + one K step so the prefetch past Kp stays inside
    return align256(((size_t)((M + BM - 1) / BM * BM) * chunk_kp(K) + 64) * sizeof(unsigned short));
}
static inline size_t ptab_bytes(const ConvGeom& g, int cw) {
    return align256(((size_t)g.B * conv_out_positions(g) / cw + PTAB_PAD) * (2 * sizeof(int)));
}
static inline size_t conv1a_wp_bytes(int M) { return align256((size_t)((M + 63) / 64 * 64) * C1_STEPS * 64); }
// extent in bytes of the tensor the gather reads (channel-sliced views: strides come from the caller)
static inline int64_t gather_extent_bytes(const ConvGeom& g, int mode, int esz = 4) {
    if (mode == MODE_FWD) return esz * ((int64_t)(g.B - 1) * g.x_bs + (int64_t)(g.Cin - 1) * g.x_cs + conv_in_positions(g));
    return esz * ((int64_t)(g.B - 1) * g.y_bs + (int64_t)(g.Cout - 1) * g.y_cs + conv_out_positions(g));
}

// ---- tile heights and split-K of the tiled kernels
// tile height: least padded M, with a small penalty for the lower arithmetic intensity of short tiles
// (192-row tiles for the chunked forward / data gradient: 2c forward +16 %; the weight gradient's measured -9 %)
static inline int choose_bm(int M, bool tall = false) {
    if (tall && M % 192 == 0) return 192;                  // one 192-row tile re-fetches the gathered operand half as often
    const int cand[4] = {128, 96, 64, 32};
    const double pen[4] = {1.00, 1.03, 1.10, 1.30};
    int best = 128;
    double bc = 1e30;
    for (int i = 0; i < 4; ++i) {
        const double c = (double)((M + cand[i] - 1) / cand[i] * cand[i]) * pen[i];
        if (c < bc) { bc = c; best = cand[i]; }
    }
    return best;
}

// choose split-K so that the grid fills the chip (256 CUs) without shredding K
static inline int choose_splits(int tiles, int K, int prec = 1, bool wgrad = false) {
    // bf16: >= 8 K steps of 32 per split (fewer, larger slabs: measured +4 % step throughput over 4);
    // fp32 parity path: 128 k per split as in the version the gradient-parity fixtures were validated with
    // The vector weight-gradient kernel keeps 4 workgroups per CU resident and its K is huge (all positions): it wants two
    // full waves of workgroups (2048; 512 left it at 2 waves per SIMD, 61 % of wave time parked).  Splits of >= 16 K steps:
    // a K step is latency-bound (~1 us) when few workgroups are resident, so the small 1x1 / 1-D layers (18 k or 1 k
    // positions, a handful of tiles) finish sooner as many short splits than as a few long ones (measured per step:
    // 48 steps 407.6 clips/s, 24: 419.0, 12: 420.1, 6: 416.2).  Forward / data gradient keep the 512-workgroup target.
    const bool wv = wgrad && prec;
    const int target = wv ? 2048 : 512;
    const int minsteps = wv ? 16 : (prec ? 8 : 4);
    const int cap = wv ? 1024 : 384;
    if (tiles >= target * 3 / 4) return 1;
    int want = (target + tiles - 1) / tiles;
    int maxs = K / (minsteps * 32);
    if (maxs < 1) maxs = 1;
    int s = want < maxs ? want : maxs;
    return s < 1 ? 1 : (s > cap ? cap : s);
}

// ---- the splits each kernel wants (and the tile counts they follow from)
// the generic kernel gets the bf16 weight gradients of the 1-D pyramid / head layers (126 positions per sample: no vector
// path): K = B * 126 positions, a few dozen tiles -- latency-bound K steps, so split down to 4 K steps per split
static inline int generic_wgrad_splits(int tiles, int K) {
    const int ms = 4;      // measured: 8 -> 474.6, 4 -> 478.3, 2 -> 478.0, 1 -> 476.3 clips/s
    const int tg = 512;
    int want = (tg + tiles - 1) / tiles, maxs = K / (ms * 32);
    if (maxs < 1) maxs = 1;
    const int s = tiles >= tg * 3 / 4 ? 1 : (want < maxs ? want : maxs);
    return s > 384 ? 384 : s;
}
// wide 1x1x1 weight gradient, row-block height in 32-row tiles: few row blocks first (each re-reads x), then little padding
// Row blocks of at most 4 x 32.  Alone, the tallest block that covers M is the fastest (Mixed_3c:
// <9> 35 us against ~45 for <4>) -- but these launches run on the weight-gradient lane BESIDE the data-gradient lane's
// kernels, and a 512-thread workgroup at 234 VGPRs (<9>) needs an EMPTY compute unit: it only got one when the main
// lane's kernel ran out of workgroups (35 us alone, 370 us beside Conv3d_2c's data gradient in the lane timeline), and the
// backlog surfaced as the step's one-lane tail.  <4> (118 VGPRs, 61 KB of LDS) fits the slot one retiring workgroup of
// the direct 3x3x3 kernel leaves (8 waves x 104-120 VGPRs, 70 KB).  Step, one box: cap 9 / 5 / 4 / 3 / 2 =
// 928 / 935 / 939 / 926 / 931 clips/s.
static inline int wgrad1x1_mt(int M) {
    const int cand[3] = {4, 3, 2};
    int mt = 2, best = 1 << 30;
    for (int i = 0; i < 3; ++i) {
        const int rb = cand[i] * 32, blocks = (M + rb - 1) / rb;
        const int cost = blocks * 256 + blocks * rb;
        if (cost < best) { best = cost; mt = cand[i]; }
    }
    return mt;
}
// one round of workgroups, >= 8 K steps per split
static inline int wgrad1x1_splits(int mt, int tiles, int K) {
    const int wgs = (mt <= 2 ? 2 : 1) * 256;              // the 64-row variant fits twice per CU: twice the loads in flight
    int splits = tiles >= wgs ? 1 : wgs / tiles;
    if (splits > K / (8 * 32)) splits = K / (8 * 32) > 0 ? K / (8 * 32) : 1;
    return splits;
}
// direct 3x3x3 weight gradient: tile height, rows per K step, K steps, wanted splits
// 64-row tiles: a 96-row tile (192 accumulator registers) spills 19 registers on 24-wide planes, and where it fits
// (12-wide planes) it measured slower (Mixed_3c b1b: 0.505 vs 0.443 ms)
// The 6x6 and 3x3 planes take 32-row tiles: half the accumulators (116-146 VGPRs instead of ~200: a workgroup that fits
// beside the other lane's, see wgrad1x1.inc) for twice the workgroups re-reading x.  Step, one box, 32-row tiles on none /
// 6x6 / 12x12 / both = 942 / 949 / 941 / 938 clips/s -- the five 6x6 layers (Mixed_4b..4f, issued beside the module's data
// gradients) gain, the 12x12 ones lose more alone than the fit returns, Conv3d_2c's runs in the one-lane tail.
static inline int wgrad_direct_rows(const ConvGeom& g) { return g.Wi == 24 ? (g.Hi % 8 == 0 ? 8 : 4) : g.Wi; }     // rows per K step
struct WgradDirectShape { int BM, steps, want; };
static inline WgradDirectShape wgrad_direct_shape(const ConvGeom& g, int M) {
    WgradDirectShape d;
    const bool planes6 = g.Wi == 6, planes3 = g.Wi == 3;
    d.BM = planes6 || planes3 ? 32 : 64;
    d.steps = planes3 ? g.B * (g.Ti / 16) : planes6 ? g.B * (g.Ti / 4) : g.B * g.Ti * (g.Hi / wgrad_direct_rows(g));       // ordered (sample, row block, t), t fastest; 6x6: four planes a step, 3x3: sixteen
    // one 512-thread workgroup per CU is resident (its registers fill the CU): aim at one full round of 256 workgroups,
    // >= 8 K steps per split, slabs <= the workspace
    const int tiles = (M + d.BM - 1) / d.BM * ((g.Cin + 31) / 32);
    int splits = tiles >= 256 ? 1 : 256 / tiles;            // never 257 workgroups: the 257th would wait for a whole round
    const int target = OTAL_OPT("OTAL_WDIRECT_BLOCKS");
    if (target > 0) splits = target / tiles > 0 ? target / tiles : 1;
    const int min_steps = planes3 || planes6 ? 4 : 8;
    if (splits > d.steps / min_steps) splits = d.steps / min_steps > 0 ? d.steps / min_steps : 1;
    d.want = splits;
    return d;
}
// Conv3d_1a's weight gradient: 2 x 2 x 48 output blocks, and
// 7 taps x S splits workgroups, two resident per CU (registers): 7 x 73 = 511 of 512 slots
// (measured on the b = 8 layer: 36 splits 0.87 ms, 73: 0.81, 109: 0.93, 146: 0.89; the pair-mode kernel: 1.05)
static inline int conv1a_wgrad_blocks(const ConvGeom& g) { return g.B * (g.To / 2) * (g.Ho / 2); }
static inline int conv1a_wgrad_splits(int nblocks) {
    const int splits = OTAL_OPT("OTAL_W1A_SPLITS") > 0 ? OTAL_OPT("OTAL_W1A_SPLITS") : 73;
    return splits > nblocks ? nblocks : splits;
}
// projection forward: split the channels so that ~512 workgroups (two per CU: 78 KB of LDS each) share the 61 MB of weights
static inline int proj_fwd_splits(int Cin, int tiles) {
    int splits = (512 + tiles - 1) / tiles;
    while (splits > 1 && (Cin % (4 * splits) != 0)) --splits;
    return splits;
}
// 1-D weight gradient: units per workgroup = (sample, chunk) units folded into one split-K slab.  Round 2 (every reduction its own launch behind
// its GEMM, one lane): 1 -> 478.4, 2 -> 475.8, 4 -> 465.7 clips/s.  Round 6 (reductions batched on the weight-gradient lane, whose
// slab traffic is what these eight launches cost -- 328 MB written, 328 MB read back per step): 1 / 2 / 4 / 8 -> 8.09 / 8.03 /
// 8.02 / 8.02 ms.  Four where there are eight units or more (two slabs at b = 8), two from four units on.
static inline int wgrad1d_upw(int units) { return units >= 8 ? 4 : units >= 4 ? 2 : 1; }

// ---- Conv3d_1a (7x7x7, stride 2, 3 input channels): direct forward, its tiled form, the weight gradient
static inline bool conv1a_half_out_ok(const ConvGeom& g, const void* y) {
    return g.y_bs % 8 == 0 && g.y_cs % 8 == 0 && (reinterpret_cast<uintptr_t>(y) & 15) == 0;
}
static inline bool conv1a_direct_eligible(const ConvGeom& g, int mode, int prec, const void* x) {
    if (!prec || mode != MODE_FWD || g.nlev > 1 || OTAL_OPT("OTAL_CONV_NO1A")) return false;
    if (g.Cin != 3 || g.kt != 7 || g.kh != 7 || g.kw != 7 || g.st != 2 || g.sh != 2 || g.sw != 2) return false;
    if (g.pt != 2 || g.ph != 2 || g.pw != 2 || g.Wi != 96 || g.Wo != C1_WO || g.Hi != 2 * g.Ho || g.Ti != 2 * g.To) return false;
    if (g.To % C1_TT || g.Ho % C1_TR || g.x_bs % 4 || g.x_cs % 4 || (reinterpret_cast<uintptr_t>(x) & 15)) return false;
    return (int64_t)g.B * g.To * g.Ho * g.Wo < (1LL << 31);
}
// 1 when the geometry is the tiled kernel's (To % 4 == 0, Ho % 4 == 0; everything else is checked by the caller)
static inline int conv1a_tile_eligible(int To, int Ho) {
    return To % C1T_TT == 0 && Ho % C1T_TR == 0 && !OTAL_OPT("OTAL_CONV_1A_NOTILE");
}
static inline bool conv1a_wgrad_eligible(const ConvGeom& g, int prec, const void* x, const void* dy) {
    if (!prec || g.nlev > 1 || OTAL_OPT("OTAL_CONV_NO1AW")) return false;
    if (g.Cin != 3 || g.Cout > 64 || g.kt != 7 || g.kh != 7 || g.kw != 7 || g.st != 2 || g.sh != 2 || g.sw != 2) return false;
    if (g.pt != 2 || g.ph != 2 || g.pw != 2 || g.Wi != 96 || g.Wo != C1_WO || g.Hi != 2 * g.Ho || g.Ti != 2 * g.To) return false;
    if (g.To % 2 || g.Ho % 2 || g.x_bs % 4 || g.x_cs % 4 || g.y_bs % 4 || g.y_cs % 4) return false;
    if ((reinterpret_cast<uintptr_t>(x) & 15) || (reinterpret_cast<uintptr_t>(dy) & 15)) return false;
    const int64_t ex = gather_extent_bytes(g, MODE_FWD), ey = gather_extent_bytes(g, MODE_DGRAD);
    return ex > 0 && ey > 0 && ex < (1LL << 31) && ey < (1LL << 31);
}

// ---- the pyramid projections (Unit3D [1,6,6] / [1,3,3], spatial_valid)
static inline bool proj_fwd_eligible(const ConvGeom& g, int mode, int prec, const void* x, const void* w) {
    if (!prec || mode != MODE_FWD || g.nlev > 1 || OTAL_OPT("OTAL_CONV_NOPROJ")) return false;
    if (g.kt != 1 || g.st != 1 || g.kh != g.Hi || g.kw != g.Wi || g.Ho != 1 || g.Wo != 1 || g.To != g.Ti) return false;
    if (g.Hi * g.Wi != PJ_HW || g.ph != 0 || g.pw != 0 || g.pt != 0 || g.Cin % 4) return false;
    // (16-byte loads at 4-byte aligned addresses are legal on gfx950 -- tools/ubench/alignprobe.hip; a weight inside the
    //  flat parameter arena is only 4-byte aligned)
    if (((uintptr_t)x & 3) || ((uintptr_t)w & 3)) return false;
    const int64_t ex = gather_extent_bytes(g, MODE_FWD), ew = 4 * (int64_t)g.Cout * g.Cin * PJ_HW;
    return ex > 0 && ex < (1LL << 31) && ew < (1LL << 31);
}
static inline bool proj_wgrad_eligible(const ConvGeom& g, int prec, const void* x, const void* dy) {
    if (!prec || g.nlev > 1 || OTAL_OPT("OTAL_CONV_NOPROJW")) return false;
    if (g.kt != 1 || g.st != 1 || g.kh != g.Hi || g.kw != g.Wi || g.Ho != 1 || g.Wo != 1 || g.To != g.Ti) return false;
    if (g.ph != 0 || g.pw != 0 || g.pt != 0 || g.Hi * g.Wi < 2) return false;          // (a 1 x 1 plane is a 1 x 1 x 1 layer: other kernels)
    if (g.To % PW_KS || g.y_cs < g.To || (g.y_cs & 3) || (g.y_bs & 3)) return false;    // whole K steps; 16-byte dc loads
    if (((uintptr_t)x & 15) || ((uintptr_t)dy & 15) || (g.x_bs & 3) || (g.x_cs & 3)) return false;
    const int64_t ex = gather_extent_bytes(g, MODE_FWD), ey = gather_extent_bytes(g, MODE_DGRAD);
    const int64_t eo = 4 * (int64_t)g.Cout * g.Cin * g.Hi * g.Wi;
    return ex > 0 && ey > 0 && ex < (1LL << 31) && ey < (1LL << 31) && eo < (1LL << 31);
}

// ---- the 1-D temporal layers (H = W = 1)
static inline bool conv1d_tile_eligible(const ConvGeom& g, int mode, int prec, const void* src, bool emask) {
    if (!prec || mode == MODE_WGRAD || OTAL_OPT("OTAL_CONV_NO1DTILE")) return false;
    if (g.Hi != 1 || g.Wi != 1 || g.Ho != 1 || g.Wo != 1 || g.kh != 1 || g.kw != 1 || g.st != 1 || g.To != g.Ti) return false;
    if (!((g.kt == 1 && g.pt == 0) || (g.kt == 3 && g.pt == 1))) return false;
    if (g.Ti > 4096) return false;
    if ((mode == MODE_FWD ? g.Cout : g.Cin) > 2048) return false;    // (the collapsed projection's 29952-row GEMM is not a temporal layer)
    const int C = mode == MODE_FWD ? g.Cin : g.Cout;
    if (C % 128) return false;                              // whole K chunks (128 channels; 64 on the 256-position maps)
    if (mode == MODE_DGRAD && emask) return false;          // the 1-D layers carry no fused ReLU / BN mask
    if (((uintptr_t)src & 3)) return false;
    const int64_t ext = gather_extent_bytes(g, mode);
    return ext > 0 && ext < (1LL << 31);
}
static inline int wgrad1d_chunks(const ConvGeom& g) { return (g.Ti + W1_TC - 1) / W1_TC; }
static inline bool wgrad1d_eligible(const ConvGeom& g, int prec, const void* x, const void* dy) {
    if (!prec || OTAL_OPT("OTAL_CONV_NOW1D")) return false;
    if (g.Hi != 1 || g.Wi != 1 || g.Ho != 1 || g.Wo != 1 || g.kh != 1 || g.kw != 1 || g.st != 1 || g.To != g.Ti) return false;
    if (!((g.kt == 1 && g.pt == 0) || (g.kt == 3 && g.pt == 1))) return false;
    if (g.Cin % 64 || (g.x_bs | g.x_cs | g.y_bs | g.y_cs) & 1) return false;
    if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(dy)) & 7) return false;
    return (int64_t)g.B * wgrad1d_chunks(g) <= 1024;
}

// ---- chunked bf16 forward / data gradient, and its 1x1x1 streaming form
static inline bool chunk_eligible(const ConvGeom& g, int mode, int prec) {
    if (!prec || mode == MODE_WGRAD) return false;
    const int C = mode == MODE_FWD ? g.Cin : g.Cout;
    if (C % 8 && !(mode == MODE_FWD && g.kw >= 3)) return false;    // forward has the kw-vector mode
    const int64_t ext = gather_extent_bytes(g, mode);
    return ext > 0 && ext < (int64_t)0xfffffff0u;       // 32-bit buffer offsets
}
static inline bool conv1x1_stream_eligible(const ConvGeom& g, int mode) {
    if (OTAL_OPT("OTAL_CONV_NO1X1STREAM")) return false;
    if (g.kt != 1 || g.kh != 1 || g.kw != 1 || g.st != 1 || g.sh != 1 || g.sw != 1 || g.nlev > 1) return false;
    const int64_t P = conv_out_positions(g);
    if (P != conv_in_positions(g) || P % 128) return false;
    const int C = mode == MODE_FWD ? g.Cin : g.Cout;
    return C % 8 == 0;
}

// ---- direct 3x3x3 forward / data gradient
static inline int direct_bm(const ConvGeom& g, int M) {
    if (M % 96 == 0) return 96;
    // one workgroup per CU and launch round: where 64-row tiles of 256 positions need a second, nearly empty round (the 6x6
    // planes of Mixed_4b..4d b1b forward: 4 x 72 = 288 workgroups) and 96-row tiles do not (3 x 72 = 216), the padded rows
    // are cheaper than the round -- forward 43 / 68 / 76 us on 64-row tiles against 56 us for Mixed_4e's 216 tiles of 96
    if (M > 96) {
        const int64_t nt = (int64_t)g.B * conv_out_positions(g) / 256;
        const int64_t w64 = (M + 63) / 64 * nt, w96 = (M + 95) / 96 * nt;
        if (w64 <= 512 && (w96 + 255) / 256 * 96 < (w64 + 255) / 256 * 64) return 96;
    }
    if (M % 64 == 0) return 64;
    // 16 .. 32 rows (data gradient of the Inception b2b layers: M = Cin = 16 / 24 / 32; forward of Mixed_3b.b2b): one 32-row
    // MFMA tile per wave.  LDS-read-bound (9 weight + 9 position fragments per 9 MFMAs), but these layers are tiny and ran
    // on the gather kernel at 25 .. 90 us for 0.1 .. 1 GFLOP of work per sample
    if (M <= 32) return 32;
    const int pad64 = (M + 63) / 64 * 64;
    return (pad64 - M) * 100 <= M * 34 ? 64 : 0;     // accept <= 34 % padded rows (Mixed_4e: 144 -> 192)
}
// positions per workgroup: 256 (8 waves), or 128 (4 waves) when 256 would leave the chip half empty (the 6x6 planes of
// Mixed_4x: 72 position tiles); 0 = too few tiles either way (no split-K on this path)
static inline int direct_bnp(const ConvGeom& g, int M) {
    const int BM = direct_bm(g, M);
    if (!BM) return 0;
    const int64_t tm = (M + BM - 1) / BM, NP = (int64_t)g.B * conv_out_positions(g);
    // (140: the 144 tiles of a one-M-tile layer on the 6x6 planes still take the 128-position form -- Mixed_4b / 4e b2b forward
    //  17.5 -> 10.1 us, 27.6 -> 12.9 us, Mixed_4b b1b data gradient 71 -> 54 us against the gather kernel; tools/micro_planes6.py)
    const int min_tiles = OTAL_OPT("OTAL_CONV_DIRECT_MINTILES");
    // 512 positions (two tiles per wave: the weight fragments are shared, the kernel turns MFMA-bound) when that still gives
    // every CU two rounds of workgroups and the tile stays inside one sample
    // (96-row tiles only: a 64-row tile of 256 positions fits TWICE per CU -- 16 waves -- and measured faster than one 512 tile)
    if (BM == 96 && conv_out_positions(g) % 512 == 0 && tm * (NP / 512) >= OTAL_OPT("OTAL_CONV_DIRECT_MINTILES512")) return 512;
    if (tm * (NP / 256) >= min_tiles) return 256;
    if (tm * (NP / 128) >= min_tiles) return 128;
    return 0;
}
static inline bool direct_eligible(const ConvGeom& g, int mode, int prec, int M) {
    if (OTAL_OPT("OTAL_CONV_NODIRECT") || !prec || mode == MODE_WGRAD || g.nlev > 1) return false;
    if (g.kt != 3 || g.kh != 3 || g.kw != 3 || g.st != 1 || g.sh != 1 || g.sw != 1 || g.pt != 1 || g.ph != 1 || g.pw != 1) return false;
    if (g.To != g.Ti || g.Ho != g.Hi || g.Wo != g.Wi || g.Wi > 24) return false;
    const int P = conv_out_positions(g);
    const int C = mode == MODE_FWD ? g.Cin : g.Cout;
    if (P % 256 || C % 16 || !direct_bnp(g, M)) return false;
    const int64_t ext = gather_extent_bytes(g, mode);
    return ext > 0 && ext < (1LL << 31);
}
static inline size_t direct_wp_bytes(const ConvGeom& g, int M, int C) {
    const int BM = direct_bm(g, M);
    return align256((size_t)((M + BM - 1) / BM * BM) * C * 27 * 2 + 1024);
}

// ---- weight gradients of the backbone
static inline bool wgrad_direct_eligible(const ConvGeom& g, int prec, const void* x, const void* dy) {
    if (!prec || OTAL_OPT("OTAL_CONV_NOWDIRECT") || g.nlev > 1) return false;
    if (g.kt != 3 || g.kh != 3 || g.kw != 3 || g.st != 1 || g.sh != 1 || g.sw != 1 || g.pt != 1 || g.ph != 1 || g.pw != 1) return false;
    if (g.To != g.Ti || g.Ho != g.Hi || g.Wo != g.Wi) return false;
    const bool planes6 = g.Wi == 6 && g.Hi == 6 && g.Ti % 4 == 0;
    const bool planes3 = g.Wi == 3 && g.Hi == 3 && g.Ti % 16 == 0;
    if (!((g.Wi == 24 && g.Hi % 4 == 0) || (g.Wi == 12 && g.Hi == 12) || planes6 || planes3) || g.Cin % 2) return false;
    if (g.Cin < (planes3 ? 32 : 64) || g.Cout < 64) return false;
    if (((uintptr_t)x & 15) || ((uintptr_t)dy & 15) || g.x_cs % 4 || g.x_bs % 4 || g.y_cs % 4 || g.y_bs % 4) return false;
    const int64_t ex = gather_extent_bytes(g, MODE_FWD), ey = gather_extent_bytes(g, MODE_DGRAD);
    return ex > 0 && ey > 0 && ex < (1LL << 31) && ey < (1LL << 31);
}
static inline bool wgrad1x1_wide_eligible(const ConvGeom& g, int prec, const void* x, const void* dy) {
    if (!prec || g.nlev > 1 || OTAL_OPT("OTAL_CONV_NOW1X1")) return false;
    if (g.kt != 1 || g.kh != 1 || g.kw != 1 || g.st != 1 || g.sh != 1 || g.sw != 1) return false;
    if (g.To != g.Ti || g.Ho != g.Hi || g.Wo != g.Wi) return false;
    if (g.Hi == 1 && g.Wi == 1) return false;               // the 1-D layers have their own weight-gradient kernel
    if (conv_out_positions(g) % 32 || (int64_t)g.Cout * g.Cin > (1 << 20)) return false;
    if (((uintptr_t)x & 3) || ((uintptr_t)dy & 3)) return false;
    const int64_t ex = gather_extent_bytes(g, MODE_FWD), ey = gather_extent_bytes(g, MODE_DGRAD);
    return ex > 0 && ey > 0 && ex < (1LL << 31) && ey < (1LL << 31);
}
// stride-2 pair mode of the vector WGRAD (Conv3d_1a): window ends must stay within 4 elements of the row
static inline bool wgrad_pair_mode(const ConvGeom& g, int prec) {
    if (!prec || g.nlev > 1) return false;
    if (g.sw != 2 || g.st > 2 || g.sh > 2 || g.kw > 7 || g.pw > 3 || g.Wo % 8 || conv_out_positions(g) % 32) return false;
    if (g.Wi - (2 * (g.Wo - 8) - g.pw + 6) < 12) return false;      // last window: elements 0..11 inside the row
    const int64_t ex = 4 * ((int64_t)(g.B - 1) * g.x_bs + (int64_t)(g.Cin - 1) * g.x_cs + conv_in_positions(g));
    const int64_t ey = 4 * ((int64_t)(g.B - 1) * g.y_bs + (int64_t)(g.Cout - 1) * g.y_cs + conv_out_positions(g));
    return ex > 0 && ey > 0 && ex < (int64_t)0xffffff00u && ey < (int64_t)0xfffffff0u;
}
// positions per vector of the vector WGRAD (0: no vector path)
static inline int wgrad_vector_width(const ConvGeom& g, int prec) {
    if (!prec) return 0;
    if (g.st != 1 || g.sh != 1 || g.sw != 1 || g.nlev > 1) return 0;
    if (g.To != g.Ti || g.Ho != g.Hi || g.Wo != g.Wi) return 0;
    if ((g.kw != 1 && g.kw != 3) || g.pw != (g.kw - 1) / 2) return 0;
    if (conv_out_positions(g) % 32) return 0;
    const int64_t ex = 4 * ((int64_t)(g.B - 1) * g.x_bs + (int64_t)(g.Cin - 1) * g.x_cs + conv_in_positions(g));
    const int64_t ey = 4 * ((int64_t)(g.B - 1) * g.y_bs + (int64_t)(g.Cout - 1) * g.y_cs + conv_out_positions(g));
    if (ex <= 0 || ey <= 0 || ex >= (int64_t)0xfffffff0u || ey >= (int64_t)0xfffffff0u) return 0;
    // a 1x1x1 kernel has no shifted tap: any 8 consecutive positions of a sample are one contiguous vector, whatever the row
    // length (6x6 planes were on 2-element vectors, 3x3 planes on the generic kernel)
    if (g.kt == 1 && g.kh == 1 && g.kw == 1) return 8;
    if (g.Wi % 8 == 0) return 8;
    if (g.Wi % 4 == 0) return 4;
    if (g.Wi % 2 == 0) return 2;
    return 0;
}

// ---- the plan
enum ConvKernel {
    CK_GENERIC,                                                                 // the tap-table kernel: any launch
    CK_PROJ, CK_CONV1A, CK_CONV1D_TILE, CK_DIRECT, CK_CHUNKED,                  // forward / data gradient
    CK_CONV1A_WGRAD, CK_PROJ_WGRAD, CK_WGRAD_DIRECT, CK_WGRAD1X1, CK_WGRAD_VECTOR, CK_WGRAD1D,   // weight gradient
};
// the kernel's name as the plans, the CPU harness and otal_conv_last_kernel() spell it
static inline const char* conv_kernel_name(int kernel) {
    switch (kernel) {
        case CK_GENERIC: return "generic";
        case CK_PROJ: return "proj";
        case CK_CONV1A: return "conv1a";
        case CK_CONV1D_TILE: return "conv1d_tile";
        case CK_DIRECT: return "direct";
        case CK_CHUNKED: return "chunked";
        case CK_CONV1A_WGRAD: return "conv1a_wgrad";
        case CK_PROJ_WGRAD: return "proj_wgrad";
        case CK_WGRAD_DIRECT: return "wgrad_direct";
        case CK_WGRAD1X1: return "wgrad1x1_wide";
        case CK_WGRAD_VECTOR: return "vector";
        case CK_WGRAD1D: return "wgrad1d";
    }
    return "?";
}
// what a persistent prologue region holds (otal_conv_prologue): nothing, the chunk table + packed weights (chunked and
// 1-D tile kernels), the position table (vector weight gradient), the direct kernel's weight pack
enum ConvPrologue { PRO_NONE = 0, PRO_CHUNK = 1, PRO_PTAB = 2, PRO_DIRECT = 3 };

// One launch as the entry points see it.  Addresses are only tested for alignment: 0 (unknown) counts as aligned.
struct ConvQuery {
    ConvGeom g;             // strides included
    int mode;
    int precision;          // the entry point's bits: 1 bf16 MFMA operands, 4 output-side tensor stored as bf16 (fwd: y,
                            // dgrad / wgrad: dy), 8 input-side tensor stored as bf16 (fwd / wgrad: x, dgrad: dx), 16 bf16 mask
    int accumulate;
    int has_mask;           // dgrad: a fused ReLU / BN mask
    uintptr_t x, w, dy, out, mask;     // out: fwd y, dgrad dx, wgrad dW
    uintptr_t prologue, prologue2;     // the caller's persistent region(s) where the step reads one (conv_launch_shape only)
    int pair;               // a pair launch: two problems of this geometry in one grid (conv_launch_shape only)
};
struct ConvStep {
    int kernel;             // ConvKernel
    int cw;                 // CK_WGRAD_VECTOR: positions per vector
    bool next;              // OTAL_E_UNSUPPORTED from this kernel moves on to the next step; otherwise its result is final
};
struct ConvPlan {
    int n;                  // 0: no kernel serves the launch
    ConvStep step[8];       // the kernels to try, in order
    int prologue;           // ConvPrologue of the geometry: a launcher reads the caller's region only when it is its own layout
};

static inline int conv_step_prologue(int kernel) {
    switch (kernel) {
        case CK_CONV1D_TILE: case CK_CHUNKED: return PRO_CHUNK;
        case CK_DIRECT: return PRO_DIRECT;
        case CK_WGRAD_VECTOR: return PRO_PTAB;
        default: return PRO_NONE;
    }
}

// the prologue a launch of this geometry uses (precision bit 0 only: one region serves fp32 and bf16 tensors)
static inline int conv_prologue_layout(const ConvGeom& g, int mode, int prec) {
    if (mode == MODE_WGRAD) return wgrad_pair_mode(g, prec) || wgrad_vector_width(g, prec) ? PRO_PTAB : PRO_NONE;
    if (proj_fwd_eligible(g, mode, prec, nullptr, nullptr)) return PRO_NONE;    // the projection reads the fp32 weights in place
    if (conv1a_direct_eligible(g, mode, prec, nullptr)) return PRO_NONE;
    if (direct_eligible(g, mode, prec, mode == MODE_FWD ? g.Cout : g.Cin)) return PRO_DIRECT;
    return chunk_eligible(g, mode, prec) ? PRO_CHUNK : PRO_NONE;
}
// bf16-stored tensors on BOTH sides of a backbone layer (fwd: x and y; dgrad: dy, dx and the ReLU mask; wgrad: x and dy)
static inline void conv_plan_half(const ConvQuery& q, ConvPlan& p) {
    const ConvGeom& g = q.g;
    const void* px = (const void*)(q.mode == MODE_DGRAD ? q.out : q.x);
    const void* py = (const void*)(q.mode == MODE_FWD ? q.out : q.dy);
    auto add = [&p](int kernel, bool next, int cw = 0) { p.step[p.n++] = ConvStep{kernel, cw, next}; };
    if (!(q.precision & 1) || !(q.precision & 4) || q.accumulate) return;
    if (((uintptr_t)px | (uintptr_t)py) & 15) return;
    if (q.mode == MODE_DGRAD && q.has_mask && (!(q.precision & 16) || (q.mask & 15))) return;
    if (g.nlev > 1) return;
    if (conv_out_positions(g) % 8 || conv_in_positions(g) % 8 || g.x_bs % 8 || g.x_cs % 8 || g.y_bs % 8 || g.y_cs % 8) return;
    if (q.mode == MODE_FWD || q.mode == MODE_DGRAD) {
        const int M = q.mode == MODE_FWD ? g.Cout : g.Cin, C = q.mode == MODE_FWD ? g.Cin : g.Cout;
        if (direct_eligible(g, q.mode, 1, M) && !(g.Wi & 1)) add(CK_DIRECT, false);
        else if (chunk_eligible(g, q.mode, 1) && C % 8 == 0 && conv_in_positions(g) == conv_out_positions(g)) add(CK_CHUNKED, false);
        return;
    }
    const int cw = wgrad_vector_width(g, 1);
    if (wgrad_direct_eligible(g, 1, px, py)) add(CK_WGRAD_DIRECT, true);
    else if (wgrad1x1_wide_eligible(g, 1, px, py)) add(CK_WGRAD1X1, true);
    if (cw) add(CK_WGRAD_VECTOR, false, cw);
}

// The kernels that serve a launch, first to last (tile shapes and splits inside one kernel: conv_launch_shape, below).
static inline ConvPlan conv_plan(const ConvQuery& q) {
    ConvPlan p = {};
    const ConvGeom& g = q.g;
    const int prec = q.precision & 1, half = (q.precision >> 2) & 1;
    p.prologue = conv_prologue_layout(g, q.mode, prec);
    if (q.precision & 8) { conv_plan_half(q, p); return p; }
    const void *x = (const void*)q.x, *w = (const void*)q.w, *dy = (const void*)q.dy, *out = (const void*)q.out;
    auto add = [&p](int kernel, bool next, int cw = 0) { p.step[p.n++] = ConvStep{kernel, cw, next}; };
    if (q.mode == MODE_WGRAD) {
        if (conv1a_wgrad_eligible(g, prec, x, dy) && (!half || g.y_bs % 8 + g.y_cs % 8 == 0)) add(CK_CONV1A_WGRAD, !half);
        if (half) return p;                                  // bf16-stored dy: the kernel above only
        if (proj_wgrad_eligible(g, prec, x, dy)) add(CK_PROJ_WGRAD, true);      // the pyramid projections: short K, no split
        if (wgrad_direct_eligible(g, prec, x, dy)) add(CK_WGRAD_DIRECT, true);  // slabs that do not fit: the kernels below
        if (wgrad1x1_wide_eligible(g, prec, x, dy)) add(CK_WGRAD1X1, true);
        if (wgrad_pair_mode(g, prec)) { add(CK_WGRAD_VECTOR, false, 8); return p; }
        if (const int cw = wgrad_vector_width(g, prec)) { add(CK_WGRAD_VECTOR, false, cw); return p; }
        if (wgrad1d_eligible(g, prec, x, dy)) add(CK_WGRAD1D, true);            // workspace too small for the slabs: generic
        add(CK_GENERIC, false);
        return p;
    }
    const int M = q.mode == MODE_FWD ? g.Cout : g.Cin;
    if (q.mode == MODE_FWD) {
        if (proj_fwd_eligible(g, q.mode, prec, x, w)) add(CK_PROJ, true);
        if (half) {         // bf16-stored y: Conv3d_1a's direct kernel and the direct 3x3x3 kernel
            if (conv1a_direct_eligible(g, q.mode, prec, x) && conv1a_half_out_ok(g, out)) add(CK_CONV1A, false);
            else if (direct_eligible(g, q.mode, prec, M) && conv1a_half_out_ok(g, out)) add(CK_DIRECT, false);
            return p;
        }
        if (conv1a_direct_eligible(g, q.mode, prec, x)) { add(CK_CONV1A, false); return p; }
    }
    if (half) return p;
    if (conv1d_tile_eligible(g, q.mode, prec, q.mode == MODE_FWD ? x : dy, q.has_mask)) add(CK_CONV1D_TILE, true);
    if (direct_eligible(g, q.mode, prec, M)) add(CK_DIRECT, false);
    else if (chunk_eligible(g, q.mode, prec)) add(CK_CHUNKED, false);
    else add(CK_GENERIC, false);        // data gradient: packs W^T first when given the natural layout
    return p;
}

// 1 when the plan for bf16-STORED tensors (precision bit 2, and bit 3 for both sides of the layer) has a kernel that stores
// them; pointer alignment and element strides that are multiples of 8 are then the caller's side of the contract.  (The
// projection kernel leads the forward chain but keeps fp32 tensors: it does not count.)
static inline int conv_half_storage(const ConvGeom& g, int mode, int precision) {
    if (!(precision & 1) || g.y_bs % 8 || g.y_cs % 8) return 0;
    ConvQuery q = {};
    q.g = g;
    q.mode = mode;
    q.precision = precision | 4;
    const ConvPlan p = conv_plan(q);
    for (int i = 0; i < p.n; ++i)
        if (p.step[i].kernel != CK_PROJ) return 1;
    return 0;
}

// ---- one step's launch: tiles, grid, split-K and the cut of the workspace, [front][slabs]
}  // namespace
struct ConvLaunchShape {    // (a type with linkage: conv_gemm.hip hands it across its two translation units)
    size_t front_bytes;     // tables and packs the launcher builds at the front: tap table, chunk table + weight pack, position
                            // table, a weight pack (0: nothing, or the caller's prologue region applies)
    size_t second_at;       // where the launch's second piece starts: the tap table behind the generic data gradient's W^T pack
                            // (forward-layout weights); a pair launch's second chunk region, or its second problem's slabs
    int N, K;               // the GEMM as this kernel sees it (kw-vector mode pads K, the weight gradient's pair mode pads N)
    int bm, tm, tn, grid[3];    // tile height, row and column tiles, the main kernel's grid (Conv3d_1a: the untiled kernel's)
    int units, splits, per_split;   // what split-K divides (K, padded K, K steps, blocks, (sample, chunk) units, channels) and how
    size_t slab_bytes;      // all slabs, behind the front
    bool refuse;            // the workspace is too small for the step: OTAL_E_UNSUPPORTED
};
namespace {

// The one carve: take n bytes off what is left of the workspace, or refuse the step.
static inline size_t shape_take(ConvLaunchShape& s, size_t& left, size_t n) {
    if (left < n) s.refuse = true; else left -= n;
    return n;
}
// The one split-K rule.  The launch wants `want` splits of `units`, each a multiple of `round` units, one slab of M x N floats
// per split in the workspace that is left (a null workspace holds nothing): clamp to what fits (fewer than two slabs, or
// not all of them where a smaller split count would not divide the units: no split), divide the units evenly, drop the
// splits the rounding left empty.  The splits are the grid's z.
static inline void fit_splits(ConvLaunchShape& s, int M, int want, int units, int round, const void* ws, size_t ws_bytes, bool all_or_none = false) {
    const size_t slab1 = (size_t)M * s.N * sizeof(float);
    if (!ws) ws_bytes = 0;
    if (want > 1 && ws_bytes < (size_t)want * slab1) want = all_or_none ? 1 : (int)(ws_bytes / slab1);
    if (want < 2) want = 1;
    s.units = units;
    s.per_split = ((units + want - 1) / want + round - 1) / round * round;
    s.splits = s.grid[2] = (units + s.per_split - 1) / s.per_split;
    s.slab_bytes = s.splits > 1 ? (size_t)s.splits * slab1 : 0;
}
// tile height and column tiles; the grid is (column tiles, row tiles, splits) unless the kernel lays it out otherwise
static inline int shape_tiles(ConvLaunchShape& s, int M, int bm, int tn) {
    s.bm = bm; s.tm = (M + bm - 1) / bm; s.tn = tn;
    s.grid[0] = tn; s.grid[1] = s.tm; s.grid[2] = 1;
    return s.tm * tn;
}

// What the launch offers: ws_bytes at ws (null: nothing).  Every step of a plan is offered the whole workspace.  (bf16
// tensors, 1x1x1 layers: where conv1x1_stream.inc serves, it shapes its own launch; this is the tile kernel behind it.)
static inline ConvLaunchShape conv_launch_shape(const ConvQuery& q, const ConvStep& step, const void* ws, size_t ws_bytes) {
    ConvLaunchShape s = {};
    const ConvGeom& g = q.g;
    const int mode = q.mode, prec = q.precision & 1, kvol = conv_kvol(g), P = (int)conv_out_positions(g);
    const int M = mode == MODE_DGRAD ? g.Cin : g.Cout, C = mode == MODE_FWD ? g.Cin : g.Cout;
    s.N = mode == MODE_FWD ? g.B * P : mode == MODE_DGRAD ? g.B * (int)conv_in_positions(g) : g.Cin * kvol;
    s.K = mode == MODE_WGRAD ? g.B * P : C * kvol;
    s.splits = 1;
    size_t left = ws ? ws_bytes : 0;
    switch (step.kernel) {
        case CK_GENERIC: {
            if (mode == MODE_DGRAD && (q.precision & 2)) s.second_at = align256((size_t)g.Cin * g.Cout * kvol * sizeof(float));
            s.front_bytes = shape_take(s, left, s.second_at + (mode != MODE_WGRAD ? tab_bytes(s.K) : 0));
            const int tiles = shape_tiles(s, M, choose_bm(M), (s.N + 127) / 128);
            fit_splits(s, M, mode == MODE_WGRAD && prec ? generic_wgrad_splits(tiles, s.K) : choose_splits(tiles, s.K, prec), s.K, 32, ws, left);
            break;
        }
        case CK_CHUNKED: case CK_CONV1D_TILE: {
            const bool kwv = mode == MODE_FWD && (C % 8) != 0, pair = step.kernel == CK_CONV1D_TILE && q.pair;
            if (kwv) s.K = g.Cin * g.kt * g.kh * 8;         // kw padded to 8 taps per (ci, dt, dh) row
            const int BMpack = choose_bm(M, !kwv);          // the weight pack's row padding (persistent regions are sized by it)
            const size_t region = chunk_tab_bytes(s.K) + chunk_wp_bytes(M, BMpack, s.K);
            s.second_at = q.prologue ? 0 : region;          // (a pair launch builds the second problem's region behind the first)
            s.front_bytes = shape_take(s, left, s.second_at + (pair && !q.prologue2 ? region : 0));
            if (step.kernel == CK_CONV1D_TILE) {
                shape_tiles(s, M, 32, g.B * ((g.Ti + 63) / 64));
                s.grid[0] = s.tm; s.grid[1] = s.tn; s.grid[2] = pair ? 2 : 1;
                break;
            }
            // bf16 tensors: the 128-row variant needs 247 registers (two workgroups per CU), the 96-row one 105 (four); rows past the
            // pack's padding read zeros through the buffer bounds check, so a different tile height may run on the same pack
            const int tiles = shape_tiles(s, M, (q.precision & 8) && BMpack == 128 ? 96 : BMpack, (s.N + 127) / 128);
            fit_splits(s, M, choose_splits(tiles, chunk_kp(s.K)), chunk_kp(s.K), 32, ws, left);
            break;
        }
        case CK_DIRECT:
            if (!direct_bnp(g, M)) { s.refuse = true; break; }
            s.front_bytes = shape_take(s, left, q.prologue ? 0 : direct_wp_bytes(g, M, C));
            shape_tiles(s, M, direct_bm(g, M), s.N / direct_bnp(g, M));
            break;
        case CK_CONV1A:         // the untiled kernel's grid; both kernels pack the weights into the same bytes
            s.front_bytes = shape_take(s, left, conv1a_wp_bytes(M));
            shape_tiles(s, M, 64, g.B * (g.To / C1_TT) * (g.Ho / C1_TR));
            break;
        case CK_PROJ: {         // a channel split that does not divide Cin is no split: all the wanted slabs, or none
            const int tiles = shape_tiles(s, M, 64, g.B * ((g.To + 63) / 64));
            fit_splits(s, M, proj_fwd_splits(g.Cin, tiles), g.Cin, 1, ws, left, true);
            s.grid[0] = s.splits; s.grid[1] = s.tm; s.grid[2] = s.tn;
            break;
        }
        case CK_CONV1A_WGRAD:
            fit_splits(s, M, conv1a_wgrad_splits(conv1a_wgrad_blocks(g)), conv1a_wgrad_blocks(g), 1, ws, left);
            s.grid[0] = 7; s.grid[1] = s.splits; s.grid[2] = 1;
            break;
        case CK_PROJ_WGRAD:
            shape_tiles(s, M, 128, (s.N + 127) / 128);
            s.grid[0] = 8 * ((s.tn + 7) / 8) * s.tm; s.grid[1] = 1;
            break;
        case CK_WGRAD_DIRECT: {
            const WgradDirectShape d = wgrad_direct_shape(g, M);
            shape_tiles(s, M, d.BM, (g.Cin + 31) / 32);
            fit_splits(s, M, d.want, d.steps, 1, ws, left);
            break;
        }
        case CK_WGRAD1X1: {
            const int tiles = shape_tiles(s, M, wgrad1x1_mt(M) * 32, (s.N + 255) / 256);
            fit_splits(s, M, wgrad1x1_splits(s.bm / 32, tiles, s.K), s.K, 32, ws, left);
            break;
        }
        case CK_WGRAD_VECTOR: {
            if (g.sw == 2) s.N = g.Cin * g.kt * g.kh * 8;   // pair mode: columns padded to 8 per (ci, dt, dh) row
            s.front_bytes = shape_take(s, left, q.prologue ? 0 : ptab_bytes(g, step.cw));
            const int tiles = shape_tiles(s, M, choose_bm(M), (s.N + 127) / 128);
            fit_splits(s, M, choose_splits(tiles, s.K, 1, true), s.K, 32, ws, left);
            break;
        }
        case CK_WGRAD1D:        // a workgroup walks wgrad1d_upw() units whatever the workspace: all the slabs (256-byte aligned), or refuse
            shape_tiles(s, M, 64, g.Cin / 64);
            s.units = g.B * wgrad1d_chunks(g);
            s.per_split = wgrad1d_upw(s.units);
            s.splits = (s.units + s.per_split - 1) / s.per_split;
            s.second_at = align256((size_t)s.splits * M * s.N * sizeof(float));
            s.slab_bytes = shape_take(s, left, s.second_at * (q.pair ? 2 : 1));
            s.grid[0] = s.splits; s.grid[1] = s.tn; s.grid[2] = s.tm * (q.pair ? 2 : 1);
            break;
        default: s.refuse = true;
    }
    return s;
}

// bytes of the geometry's prologue region (0: none): the front the kernel of that layout would otherwise build
static inline size_t conv_prologue_bytes(const ConvGeom& g, int mode, int prec) {
    const int layout = conv_prologue_layout(g, mode, prec);
    ConvQuery q = {};
    q.g = g; q.mode = mode; q.precision = prec;
    const ConvStep step = {layout == PRO_CHUNK ? CK_CHUNKED : layout == PRO_PTAB ? CK_WGRAD_VECTOR : CK_DIRECT, g.sw == 2 ? 8 : wgrad_vector_width(g, prec), false};
    return layout == PRO_NONE ? 0 : conv_launch_shape(q, step, &q, ~(size_t)0 >> 1).front_bytes;
}

// Bytes of workspace with which every kernel of this geometry's plans takes all the splits it wants: the largest front plus
// slabs over the steps of the plans for contiguous, aligned tensors -- fp32 and bf16 operands, fp32- and bf16-stored
// tensors, the data gradient from forward-layout weights.  (A pair launch of a 1-D layer takes twice its bytes; a strided
// or misaligned view whose plan differs from the contiguous one may be served with fewer splits at this size.)
static inline size_t conv_workspace_bytes(const ConvGeom& geom, int mode) {
    ConvQuery q = {};
    q.g = geom; q.mode = mode;
    q.g.x_cs = conv_in_positions(geom); q.g.x_bs = geom.Cin * q.g.x_cs;
    q.g.y_cs = conv_out_positions(geom); q.g.y_bs = geom.Cout * q.g.y_cs;
    size_t need = 0;
    for (const int precision : {0, 1, 1 | 4, 1 | 4 | 8 | 16}) {
        q.precision = precision | (mode == MODE_DGRAD ? 2 : 0);
        const ConvPlan p = conv_plan(q);
        for (int j = 0; j < p.n; ++j) {
            const ConvLaunchShape s = conv_launch_shape(q, p.step[j], &q, ~(size_t)0 >> 1);
            if (s.front_bytes + s.slab_bytes > need) need = s.front_bytes + s.slab_bytes;
        }
    }
    return need;
}

}  // namespace
