// opental_amd/csrc/conv_wgrad_direct.inc -- included by conv_gemm.hip inside its anonymous namespace.
//
// Direct WEIGHT GRADIENT of the stride-1 SAME 3x3x3 layers of the I3D backbone on 24x24 / 12x12 / 6x6 planes
// (Conv3d_2c, Mixed_3b/3c b1b, b2b; autograd of AFSD/common/i3d_backbone.py:33-43):
//
//     dW[co][ci][dt][dh][dw] = sum over (b,t,h,w)  dy[b][co][t][h][w] * x[b][ci][t+dt-1][h+dh-1][w+dw-1]
//
// The vector kernel above gathers every x element once PER TAP (27 times through L1) and is bound by the texture
// addresser: 28 wide loads per 24 MFMAs.  Here a workgroup owns the tile (BM output channels) x (32 input channels x
// ALL 27 taps) and walks over a slice of the positions in K steps of FOUR ROWS of one (sample, t) plane:
//   * dy  : the step's BM x (4 W) values, bf16, K(position)-contiguous in LDS -> A fragments by ds_read_b128;
//   * x   : the step's receptive field -- 3 planes x 6 rows x (W + 2) columns, zero border included -- staged ONCE as
//           [cell][32 channels] bf16 (64 B per cell).  The B fragment of tap (dt,dh,dw) for K positions p..p+7 is
//           the 8 cells at (p + tap shift): ds_read_b64_tr_b16 transposes [4 cells][16 channels] blocks on the fly, each
//           quad of lanes supplying the address of ITS cell, so a tap is one uniform byte offset added to a per-lane
//           constant and out-of-range taps simply read the zero border (no masks, no per-tap gather).
// Per K step and workgroup: ~90 wide loads against ~480 MFMAs.  Split-K over position ranges; slabs reduced in a fixed
// order by splitk_reduce_kernel (deterministic).
struct WD3Args {
    ConvArgs c;        // geometry, x, dy, out / slab, M = Cout, N = Cin * 27, splits, flags
    int HB;            // row blocks per plane (H / rows per K step)
    int steps;         // K steps in all: B * HB * T, ordered (sample, row block, t) with t fastest
    int sps;           // K steps per split
};

typedef short v4s16 __attribute__((ext_vector_type(4)));
typedef unsigned wd3_u32x4 __attribute__((ext_vector_type(4)));

// epilogue of the direct weight-gradient kernels: column (tap, ci) of the tile is column ci * 27 + tap of dW, and wave w owns
// taps w, w + 8, w + 16 (, w + 24 for waves 0..2) -- a lane's 4-byte values land 108 bytes apart in a row of dW.  The tile
// therefore goes through LDS, ROWS (8 or 16, what the kernel's allocation holds) rows of 32 ci x 27 taps at a time, and
// leaves as whole rows: 3456 contiguous bytes each, 16-byte stores.  Split-K partial sums are written the same way into
// slabs of dW's own layout [split][m][ci][tap], so the ordinary reduction (recorded and batched with the step's others when
// the caller defers reductions) sums them.  (Until round 6 the slabs were tap-major, [split][m][tap][ci] -- 128-byte runs --
// and every launch was followed by its own transposing reduction: eleven launches of 10-47 us on the weight-gradient lane.)
template <int MT, int ROWS>
__device__ __forceinline__ void wd3_epilogue(const ConvArgs& a, const f32x16 (&acc)[MT][4], int ci0, int m0, int split, int wave, int lane,
                                             unsigned char* smem) {
    constexpr int RP = 868;                                 // floats per staged row (864 + 4: the two half-waves' rows 4 apart do not share banks)
    static_assert(ROWS == 8 || ROWS == 16, "rows per phase");
    const ConvGeom& g = a.g;
    const bool four = wave < 3;
    const bool slabs = a.splits > 1;
    const auto ro = __builtin_amdgcn_make_buffer_rsrc(slabs ? a.slab : a.out, 0, (int)(slabs ? a.slab_bytes : a.out_bytes), 0x00020000);
    const bool accum = !slabs && (a.flags & EPI_ACCUM);
    float* const stage = reinterpret_cast<float*>(smem);
    const int tid = wave * 64 + lane;
    const int ncol = min(32, g.Cin - ci0) * 27;             // floats of a row that exist
    const bool v4 = (g.Cin & 3) == 0;                       // rows of dW start 16-byte aligned and hold whole quads
    const unsigned row0 = (unsigned)(slabs ? split : 0) * (unsigned)a.M;
#pragma unroll
    for (int i = 0; i < MT; ++i) {
#pragma unroll
        for (int ph = 0; ph < 32 / ROWS; ++ph) {
            __syncthreads();                                // the K loop's (or the previous phase's) readers are done
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (j == 3 && !four) continue;
                const int tau = wave + 8 * j;
#pragma unroll
                for (int q = 0; q < ROWS / 2; ++q) {
                    const int r = ph * (ROWS / 2) + q;      // accumulator register: row (r & 3) + 8 (r >> 2) + 4 (lane >> 5) of the 32
                    const int rl = (r & 3) + 8 * ((r >> 2) % (ROWS / 8)) + 4 * (lane >> 5);
                    stage[rl * RP + (lane & 31) * 27 + tau] = acc[i][j][r];
                }
            }
            __syncthreads();
            const int mrow = m0 + i * 32 + ph * ROWS;
            if (v4) {
                for (int idx = tid; idx < ROWS * 216; idx += 512) {
                    const int rl = idx / 216, c = (idx - rl * 216) * 4;
                    const int m = mrow + rl;
                    if (c >= ncol || m >= a.M) continue;
                    float4 v = *reinterpret_cast<const float4*>(stage + rl * RP + c);
                    const unsigned off = ((row0 + (unsigned)m) * (unsigned)a.N + (unsigned)(ci0 * 27 + c)) * 4u;
                    if (accum) {
                        const Words4 o = __builtin_bit_cast(Words4, __builtin_amdgcn_raw_buffer_load_b128(ro, off, 0, 0));
                        v.x += __uint_as_float(o.a); v.y += __uint_as_float(o.b); v.z += __uint_as_float(o.c); v.w += __uint_as_float(o.d);
                    }
                    Words4 w;
                    w.a = __float_as_uint(v.x); w.b = __float_as_uint(v.y); w.c = __float_as_uint(v.z); w.d = __float_as_uint(v.w);
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(wd3_u32x4, w), ro, off, 0, 0);
                }
            } else {
                for (int idx = tid; idx < ROWS * 864; idx += 512) {
                    const int rl = idx / 864, c = idx - rl * 864;
                    const int m = mrow + rl;
                    if (c >= ncol || m >= a.M) continue;
                    float v = stage[rl * RP + c];
                    const unsigned off = ((row0 + (unsigned)m) * (unsigned)a.N + (unsigned)(ci0 * 27 + c)) * 4u;
                    if (accum) v += __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(ro, off, 0, 0));
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), ro, off, 0, 0);
                }
            }
        }
    }
}

// K-step order: t runs fastest for a fixed (sample, row block), so consecutive steps share two of their three planes.
// The x planes live in a RING of four LDS slabs (slab = 6 rows x (W + 2) cells x 32 channels): step t reads planes
// t-1, t, t+1 from slots t, t+1, t+2 (mod 4) while plane t+2 is prefetched into the fourth -- every x element is loaded
// 1.5 times (row halo) instead of 4.5 times, and a step moves 43 KB instead of 80 KB through L1 (the first version,
// re-staging three planes per step, ran at the HBM-bound ~10 B/clk/CU).  At the start of a split and at every (sample,
// row block) change the three planes are staged synchronously (once per T steps).
// H: x and dy are STORED as bf16.  x: (row, quad of columns, channel pair) items as before, two 8-byte loads each, transposed
// into the [cell][32 channels] slab by pair_lo / pair_hi (no conversion); dy: 16-byte loads of eight positions straight into
// the K-contiguous tile.  Same operands, same accumulation order as the fp32-tensor kernel on the same values.
template <int BM, int PW, int PR, bool HS = false>
__global__ __launch_bounds__(512) void conv3_wgrad_direct_kernel(const WD3Args d) {
    constexpr int KS = PR * PW, NS = KS / 16, MT = BM / 32;        // PR rows of a plane per K step (24-wide: 4, 12-wide: the whole plane)
    constexpr int CR = PR + 2, CC = PW + 2;
    constexpr int SLAB = CR * CC * 64, XB = 4 * SLAB;       // bytes of one plane slab, of the ring
    constexpr int AP = KS * 2 + 16, AB = BM * AP;           // dy tile: row pitch (conflict-free ds_read_b128), bytes
    constexpr int QW = PW / 4;
    constexpr int ESZ = HS ? 2 : 4, AV = HS ? 8 : 4;           // bytes per element; dy positions per 16-byte load
    constexpr int S_ITEMS = CR * QW * 16, S_ITERS = (S_ITEMS + 511) / 512;          // (row, quad of columns, channel pair) of a slab
    constexpr int A_ITEMS = BM * (KS / AV), A_ITERS = (A_ITEMS + 511) / 512;         // (row, quad [octet] of positions)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];            // [4][SLAB] then [2][AB]
    const ConvArgs& a = d.c;
    const ConvGeom& g = a.g;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const TileId tile = xcd_tile(false);                    // x: 32-channel block of Cin, y: BM block of Cout, z: split
    const int ci0 = tile.x * 32, m0 = tile.y * BM, split = tile.z;
    const int q_begin = split * d.sps, q_end = min(d.steps, q_begin + d.sps);
    const int W = g.Wi, HW = g.Hi * g.Wi, T = g.Ti, H = g.Hi;
    const auto rxs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.x), 0, (int)a.src_bytes, 0x00020000);
    const auto rdy = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.dy), 0, (int)a.dy_bytes, 0x00020000);

    // ---- zero the ring once: border columns are never written again
    for (int i = tid; i < XB / 16; i += 512) reinterpret_cast<uint4*>(smem)[i] = make_uint4(0u, 0u, 0u, 0u);

    // ---- per-thread staging items (fixed for the whole launch)
    int srel[S_ITERS], slds[S_ITERS];
    unsigned sim[S_ITERS];
#pragma unroll
    for (int i = 0; i < S_ITERS; ++i) {
        const int item = tid + 512 * i;
        const int p = item & 15, rest = item >> 4;
        const int q = rest % QW, r = rest / QW;
        const bool used = item < S_ITEMS && ci0 + 2 * p + 1 < g.Cin;
        srel[i] = (int)(((int64_t)(2 * p) * g.x_cs + (r - 1) * W + 4 * q) * ESZ);
        sim[i] = (unsigned)(r == 0) | ((unsigned)(r == CR - 1) << 1) | ((unsigned)(!used) << 2);
        slds[i] = (r * CC + 4 * q + 1) * 64 + p * 4;
    }
    unsigned avo[A_ITERS];
    int alds[A_ITERS];
#pragma unroll
    for (int j = 0; j < A_ITERS; ++j) {
        const int item = tid + 512 * j;
        const int m = item / (KS / AV), qd = item - m * (KS / AV);
        const bool used = item < A_ITEMS && m0 + m < a.M;
        avo[j] = used ? (unsigned)(((int64_t)(m0 + m) * g.y_cs + AV * qd) * ESZ) : 0xffffffffu;
        alds[j] = m * AP + qd * (AV * 2);
    }
    // ---- B-fragment cell addresses of this lane inside a slab: K position p = 16 s + 8 (lane >> 5) + 4 h + ((lane & 15) >> 2)
    int lb[NS][2];
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int p = 16 * s + 8 * (lane >> 5) + 4 * h + ((lane & 15) >> 2);
            lb[s][h] = ((p / PW) * CC + (p % PW)) * 64 + ((lane >> 4) & 1) * 32 + (lane & 3) * 8;
        }
    // this wave's taps: wave, wave + 8, wave + 16 (, wave + 24 for waves 0..2)
    int tapdt[4], tapin[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int tau = min(wave + 8 * j, 26);
        const int dt = tau / 9, dh = (tau / 3) % 3, dw = tau % 3;
        tapdt[j] = dt;
        tapin[j] = (dh * CC + dw) * 64;
    }
    const bool four = wave < 3;

    unsigned rx[S_ITERS][2][4];
    Words4 ra[A_ITERS];
    auto load_slab = [&](int b, int hb, int plane) {        // rows hb*4 - 1 .. hb*4 + 4 of plane `plane` (zeros outside the tensor)
        const int h0 = hb * PR;
        const unsigned smask = (unsigned)(h0 == 0) | ((unsigned)(h0 + PR == H) << 1) | 4u | ((plane < 0 || plane >= T) ? 8u : 0u);
        const int xbase = (int)(((int64_t)b * g.x_bs + (int64_t)ci0 * g.x_cs + (int64_t)plane * HW + h0 * W) * ESZ);
#pragma unroll
        for (int i = 0; i < S_ITERS; ++i) {
            const unsigned vo = ((sim[i] | 8u) & smask) ? a.src_bytes : (unsigned)(srel[i] + xbase);
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                if constexpr (HS) {
                    const Words2 v = __builtin_bit_cast(Words2, __builtin_amdgcn_raw_buffer_load_b64(rxs, vo, h ? (int)(g.x_cs * 2) : 0, 0));
                    rx[i][h][0] = v.a; rx[i][h][1] = v.b;
                } else {
                    const Words4 v = __builtin_bit_cast(Words4, __builtin_amdgcn_raw_buffer_load_b128(rxs, vo, h ? (int)(g.x_cs * 4) : 0, 0));
                    rx[i][h][0] = v.a; rx[i][h][1] = v.b; rx[i][h][2] = v.c; rx[i][h][3] = v.d;
                }
            }
        }
    };
    auto store_slab = [&](int slot) {
        unsigned char* X = smem + slot * SLAB;
#pragma unroll
        for (int i = 0; i < S_ITERS; ++i) {
            if (S_ITEMS % 512 != 0 && tid + 512 * i >= S_ITEMS) continue;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if constexpr (HS)
                    *reinterpret_cast<unsigned*>(X + slds[i] + e * 64) =
                        (e & 1) ? pair_hi(rx[i][0][e >> 1], rx[i][1][e >> 1]) : pair_lo(rx[i][0][e >> 1], rx[i][1][e >> 1]);
                else
                    *reinterpret_cast<unsigned*>(X + slds[i] + e * 64) =
                        cvt_pk_bf16(__uint_as_float(rx[i][0][e]), __uint_as_float(rx[i][1][e]));
            }
        }
    };
    auto load_dy = [&](int b, int hb, int t) {
        const int ybase = (int)(((int64_t)b * g.y_bs + (int64_t)t * HW + hb * PR * W) * ESZ);
#pragma unroll
        for (int j = 0; j < A_ITERS; ++j)
            ra[j] = __builtin_bit_cast(Words4, __builtin_amdgcn_raw_buffer_load_b128(rdy, avo[j], ybase, 0));
    };
    auto store_dy = [&](int buf) {
        unsigned char* A = smem + XB + buf * AB;
#pragma unroll
        for (int j = 0; j < A_ITERS; ++j) {
            if (A_ITEMS % 512 != 0 && tid + 512 * j >= A_ITEMS) continue;
            if constexpr (HS) {
                *reinterpret_cast<Words4*>(A + alds[j]) = ra[j];
            } else {
                Words2 pk;
                pk.a = cvt_pk_bf16(__builtin_bit_cast(float, ra[j].a), __builtin_bit_cast(float, ra[j].b));
                pk.b = cvt_pk_bf16(__builtin_bit_cast(float, ra[j].c), __builtin_bit_cast(float, ra[j].d));
                *reinterpret_cast<Words2*>(A + alds[j]) = pk;
            }
        }
    };

    f32x16 acc[MT][4];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    typedef __attribute__((address_space(3))) unsigned char lds_byte;
    lds_byte* const lds0 = (lds_byte*)smem;

    // step q -> (sample b, row block hb, plane t), t fastest
    int sb, shb, stt;
    {
        const int r = q_begin / T;
        stt = q_begin - r * T;
        sb = r / d.HB;
        shb = r - sb * d.HB;
    }
    bool warm = true;
    if (q_begin < q_end) {
        load_dy(sb, shb, stt);
        store_dy(0);
    }
    for (int q = q_begin; q < q_end; ++q) {
        const int buf = (q - q_begin) & 1;
        if (warm) {                                         // planes t-1, t, t+1 of a new (sample, row block) run
            __syncthreads();                                // nobody still reads the slots (nor the zero fill is pending)
#pragma unroll 1
            for (int pl = 0; pl < 3; ++pl) {
                load_slab(sb, shb, stt - 1 + pl);
                store_slab((stt + pl) & 3);
            }
        }
        __syncthreads();                                    // staged tiles of this step are visible
        const bool more = q + 1 < q_end;
        const bool same_run = more && stt + 1 < T;
        int nb = sb, nhb = shb, nt = stt + 1;
        if (nt == T) { nt = 0; if (++nhb == d.HB) { nhb = 0; ++nb; } }
        int toff[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) toff[j] = ((stt + tapdt[j]) & 3) * SLAB + tapin[j];
        const unsigned char* const A = smem + XB + buf * AB;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            if (s == 0) {
                if (more) load_dy(nb, nhb, nt);
                if (same_run) load_slab(sb, shb, stt + 2);  // the plane the NEXT step adds, into the free slot
            }
            bf16x8 av[MT];
#pragma unroll
            for (int i = 0; i < MT; ++i)
                av[i] = *reinterpret_cast<const bf16x8*>(A + (i * 32 + (lane & 31)) * AP + (s * 16 + 8 * (lane >> 5)) * 2);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (j == 3 && !four) continue;
                const v4s16 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                    (__attribute__((address_space(3))) v4s16*)(lds0 + lb[s][0] + toff[j]));
                const v4s16 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                    (__attribute__((address_space(3))) v4s16*)(lds0 + lb[s][1] + toff[j]));
                const bf16x8 bv = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
#pragma unroll
                for (int i = 0; i < MT; ++i)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av[i], bv, acc[i][j], 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        if (more) store_dy(buf ^ 1);
        if (same_run) store_slab((stt + 3) & 3);
        warm = more && !same_run;
        sb = nb; shb = nhb; stt = nt;
    }

    wd3_epilogue<MT, (XB + 2 * AB >= 16 * 868 * 4 ? 16 : 8)>(a, acc, ci0, m0, split, wave, lane, smem);
}

// ---- 6x6 planes (Mixed_4b .. 4f, b1b / b2b): a plane holds only 36 positions, so a K step is FOUR whole planes of one
// sample (144 positions = 9 MFMA K blocks, contiguous in dy).  The x planes live in a ring of 16 slabs of 8 x 8 cells
// (4 KB each, zero border): plane pl sits in slot (pl + 1) & 15, so the B fragment of tap (dt, dh, dw) for the position
// (plane j, h, w) of the step is at  (lane constant + ((t0 + dt) * 4 KB + tap shift)) & 0xffff -- one add and one and.
// Planes are staged in aligned groups of four (4k - 1 .. 4k + 2): step k reads groups k and k + 1 while group k + 2 is
// prefetched; every x element is loaded exactly once per (Cout tile) workgroup.
template <int BM, bool H = false>
__global__ __launch_bounds__(512) void conv3_wgrad_planes6_kernel(const WD3Args d) {
    constexpr int KS = 144, NS = 9, MT = BM / 32, PP = 36;
    constexpr int SLAB = 4096, XB = 16 * SLAB;
    constexpr int AP = KS * 2 + 16, AB = BM * AP;
    constexpr int ESZ = H ? 2 : 4, AV = H ? 8 : 4;           // H: bf16-stored x and dy (see conv3_wgrad_direct_kernel)
    constexpr int S_ITEMS = 4 * 9 * 16, S_ITERS = (S_ITEMS + 511) / 512;           // (plane of the group, quad of positions, channel pair)
    constexpr int A_ITEMS = BM * (KS / AV), A_ITERS = (A_ITEMS + 511) / 512;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];            // [16][SLAB] then [2][AB]
    const ConvArgs& a = d.c;
    const ConvGeom& g = a.g;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const TileId tile = xcd_tile(false);
    const int ci0 = tile.x * 32, m0 = tile.y * BM, split = tile.z;
    const int q_begin = split * d.sps, q_end = min(d.steps, q_begin + d.sps);
    const int T = g.Ti, KT = T >> 2;                        // steps per sample
    const auto rxs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.x), 0, (int)a.src_bytes, 0x00020000);
    const auto rdy = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.dy), 0, (int)a.dy_bytes, 0x00020000);
    for (int i = tid; i < XB / 16; i += 512) reinterpret_cast<uint4*>(smem)[i] = make_uint4(0u, 0u, 0u, 0u);

    int srel[S_ITERS], slds[S_ITERS];
    unsigned scell[S_ITERS];
    bool sused[S_ITERS];
#pragma unroll
    for (int i = 0; i < S_ITERS; ++i) {
        const int item = tid + 512 * i;
        const int cp = item & 15, rest = item >> 4;
        const int q = rest % 9, j = (rest / 9) & 3;
        sused[i] = item < S_ITEMS && ci0 + 2 * cp + 1 < g.Cin;
        srel[i] = (int)(((int64_t)(2 * cp) * g.x_cs + j * PP + 4 * q) * ESZ);
        slds[i] = j * SLAB + cp * 4;
        unsigned cells = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int p = 4 * q + e;
            cells |= (unsigned)((p / 6 + 1) * 8 + p % 6 + 1) << (8 * e);
        }
        scell[i] = cells;
    }
    unsigned avo[A_ITERS];
    int alds[A_ITERS];
#pragma unroll
    for (int j = 0; j < A_ITERS; ++j) {
        const int item = tid + 512 * j;
        const int m = item / (KS / AV), qd = item - m * (KS / AV);
        const bool used = item < A_ITEMS && m0 + m < a.M;
        avo[j] = used ? (unsigned)(((int64_t)(m0 + m) * g.y_cs + AV * qd) * ESZ) : 0xffffffffu;
        alds[j] = m * AP + qd * (AV * 2);
    }
    int lb[NS][2];
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int p = 16 * s + 8 * (lane >> 5) + 4 * h + ((lane & 15) >> 2);
            const int j = p / PP, r = p - j * PP;
            lb[s][h] = j * SLAB + ((r / 6) * 8 + r % 6) * 64 + ((lane >> 4) & 1) * 32 + (lane & 3) * 8;
        }
    int tapdt[4], tapin[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int tau = min(wave + 8 * j, 26);
        const int dt = tau / 9, dh = (tau / 3) % 3, dw = tau % 3;
        tapdt[j] = dt;
        tapin[j] = (dh * 8 + dw) * 64;
    }
    const bool four = wave < 3;

    unsigned rx[S_ITERS][2][4];
    Words4 ra[A_ITERS];
    auto load_group = [&](int b, int k) {                   // planes 4k - 1 .. 4k + 2 of sample b (zeros outside 0 .. T-1)
        const int xbase = (int)(((int64_t)b * g.x_bs + (int64_t)ci0 * g.x_cs + (int64_t)(4 * k - 1) * PP) * ESZ);
#pragma unroll
        for (int i = 0; i < S_ITERS; ++i) {
            const int pl = 4 * k - 1 + (slds[i] >> 12);
            const unsigned vo = (!sused[i] || pl < 0 || pl >= T) ? a.src_bytes : (unsigned)(srel[i] + xbase);
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                if constexpr (H) {
                    const Words2 v = __builtin_bit_cast(Words2, __builtin_amdgcn_raw_buffer_load_b64(rxs, vo, h ? (int)(g.x_cs * 2) : 0, 0));
                    rx[i][h][0] = v.a; rx[i][h][1] = v.b;
                } else {
                    const Words4 v = __builtin_bit_cast(Words4, __builtin_amdgcn_raw_buffer_load_b128(rxs, vo, h ? (int)(g.x_cs * 4) : 0, 0));
                    rx[i][h][0] = v.a; rx[i][h][1] = v.b; rx[i][h][2] = v.c; rx[i][h][3] = v.d;
                }
            }
        }
    };
    auto store_group = [&](int k) {
        unsigned char* X = smem + ((4 * k) & 15) * SLAB;
#pragma unroll
        for (int i = 0; i < S_ITERS; ++i) {
            if (tid + 512 * i >= S_ITEMS) continue;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                unsigned* dst = reinterpret_cast<unsigned*>(X + slds[i] + ((scell[i] >> (8 * e)) & 255u) * 64);
                if constexpr (H) *dst = (e & 1) ? pair_hi(rx[i][0][e >> 1], rx[i][1][e >> 1]) : pair_lo(rx[i][0][e >> 1], rx[i][1][e >> 1]);
                else *dst = cvt_pk_bf16(__uint_as_float(rx[i][0][e]), __uint_as_float(rx[i][1][e]));
            }
        }
    };
    auto load_dy = [&](int b, int k) {
        const int ybase = (int)(((int64_t)b * g.y_bs + (int64_t)(4 * k) * PP) * ESZ);
#pragma unroll
        for (int j = 0; j < A_ITERS; ++j)
            ra[j] = __builtin_bit_cast(Words4, __builtin_amdgcn_raw_buffer_load_b128(rdy, avo[j], ybase, 0));
    };
    auto store_dy = [&](int buf) {
        unsigned char* A = smem + XB + buf * AB;
#pragma unroll
        for (int j = 0; j < A_ITERS; ++j) {
            if (A_ITEMS % 512 != 0 && tid + 512 * j >= A_ITEMS) continue;
            if constexpr (H) {
                *reinterpret_cast<Words4*>(A + alds[j]) = ra[j];
            } else {
                Words2 pk;
                pk.a = cvt_pk_bf16(__builtin_bit_cast(float, ra[j].a), __builtin_bit_cast(float, ra[j].b));
                pk.b = cvt_pk_bf16(__builtin_bit_cast(float, ra[j].c), __builtin_bit_cast(float, ra[j].d));
                *reinterpret_cast<Words2*>(A + alds[j]) = pk;
            }
        }
    };

    f32x16 acc[MT][4];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    typedef __attribute__((address_space(3))) unsigned char lds_byte;
    lds_byte* const lds0 = (lds_byte*)smem;

    int sb = q_begin / KT, sk = q_begin - sb * KT;
    bool warm = true;
    if (q_begin < q_end) {
        load_dy(sb, sk);
        store_dy(0);
    }
    for (int q = q_begin; q < q_end; ++q) {
        const int buf = (q - q_begin) & 1;
        if (warm) {                                         // groups k and k + 1 of a new sample (or of the split's first step)
            __syncthreads();
#pragma unroll 1
            for (int gk = 0; gk < 2; ++gk) {
                load_group(sb, sk + gk);
                store_group(sk + gk);
            }
        }
        __syncthreads();
        const bool more = q + 1 < q_end;
        const bool same_run = more && sk + 1 < KT;
        int nb = sb, nk = sk + 1;
        if (nk == KT) { nk = 0; ++nb; }
        int toff[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) toff[j] = ((4 * sk + tapdt[j]) & 15) * SLAB + tapin[j];
        const unsigned char* const A = smem + XB + buf * AB;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            if (s == 0) {
                if (more) load_dy(nb, nk);
                if (same_run) load_group(sb, sk + 2);
            }
            bf16x8 av[MT];
#pragma unroll
            for (int i = 0; i < MT; ++i)
                av[i] = *reinterpret_cast<const bf16x8*>(A + (i * 32 + (lane & 31)) * AP + (s * 16 + 8 * (lane >> 5)) * 2);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (j == 3 && !four) continue;
                const v4s16 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                    (__attribute__((address_space(3))) v4s16*)(lds0 + ((lb[s][0] + toff[j]) & (XB - 1))));
                const v4s16 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                    (__attribute__((address_space(3))) v4s16*)(lds0 + ((lb[s][1] + toff[j]) & (XB - 1))));
                const bf16x8 bv = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
#pragma unroll
                for (int i = 0; i < MT; ++i)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av[i], bv, acc[i][j], 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        if (more) store_dy(buf ^ 1);
        if (same_run) store_group(sk + 2);
        warm = more && !same_run;
        sb = nb; sk = nk;
    }
    wd3_epilogue<MT, 16>(a, acc, ci0, m0, split, wave, lane, smem);
}

// ---- 3x3 planes (Mixed_5b / 5c, b1b / b2b): a plane holds 9 positions, a sample 32 planes -- a K step is SIXTEEN whole
// planes of one sample (144 positions = 9 MFMA K blocks, contiguous in dy), and the x operand of a step is its own slab of
// 18 planes (the 16 and one either side; zeros outside the sample) of 5 x 5 cells (zero border) x 32 channels: 28.8 KB.  No ring:
// a sample is two steps, so the slab of step q + 1 is simply staged into the other buffer while step q computes (the two
// halo planes are loaded twice: 12 %).  The B fragment of tap (dt, dh, dw) is a per-lane constant plus one per-wave offset.
// The generic gather kernel ran these four layers at 90-110 TFLOP/s (K = 2304 positions only: every launch is a handful
// of K steps whose 27-fold gather of x is the work).
template <int BM, bool H = false>
__global__ __launch_bounds__(512) void conv3_wgrad_planes3_kernel(const WD3Args d) {
    constexpr int KS = 144, NS = 9, MT = BM / 32, PP = 9, PS = 16;
    constexpr int SLAB = 25 * 64, XB = (PS + 2) * SLAB;     // one plane, one step's slab
    constexpr int AP = KS * 2 + 16, AB = BM * AP;
    constexpr int ESZ = H ? 2 : 4, AV = H ? 8 : 4;
    constexpr int QN = 42;                                   // quads of positions -12 .. 155 relative to the step's first position
    constexpr int S_ITEMS = QN * 16, S_ITERS = (S_ITEMS + 511) / 512;               // (quad of positions, channel pair)
    constexpr int A_ITEMS = BM * (KS / AV), A_ITERS = (A_ITEMS + 511) / 512;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];            // [2][XB] then [2][AB]
    const ConvArgs& a = d.c;
    const ConvGeom& g = a.g;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const TileId tile = xcd_tile(false);
    const int ci0 = tile.x * 32, m0 = tile.y * BM, split = tile.z;
    const int q_begin = split * d.sps, q_end = min(d.steps, q_begin + d.sps);
    const int T = g.Ti, KT = T / PS;                         // steps per sample
    const auto rxs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.x), 0, (int)a.src_bytes, 0x00020000);
    const auto rdy = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.dy), 0, (int)a.dy_bytes, 0x00020000);
    for (int i = tid; i < 2 * XB / 16; i += 512) reinterpret_cast<uint4*>(smem)[i] = make_uint4(0u, 0u, 0u, 0u);   // the borders stay zero

    int srel[S_ITERS], sq[S_ITERS];
    unsigned scell[S_ITERS][2];                              // LDS byte offsets of the quad's four positions (0xffff: outside the slab)
    bool sused[S_ITERS];
#pragma unroll
    for (int i = 0; i < S_ITERS; ++i) {
        const int item = tid + 512 * i;
        const int cp = item & 15, qd = item >> 4;
        sused[i] = item < S_ITEMS && ci0 + 2 * cp + 1 < g.Cin;
        sq[i] = qd;
        srel[i] = (int)(((int64_t)(2 * cp) * g.x_cs + 4 * qd - 12) * ESZ);
        scell[i][0] = scell[i][1] = 0u;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int pos = 4 * qd - 12 + e + PP;            // 0 .. 161 inside the 18 planes
            unsigned off = 0xffffu;
            if (item < S_ITEMS && pos >= 0 && pos < (PS + 2) * PP) {
                const int slot = pos / PP, r = pos - slot * PP;
                off = (unsigned)(slot * SLAB + ((r / 3 + 1) * 5 + r % 3 + 1) * 64 + cp * 4);
            }
            scell[i][e >> 1] |= off << (16 * (e & 1));
        }
    }
    unsigned avo[A_ITERS];
    int alds[A_ITERS];
#pragma unroll
    for (int j = 0; j < A_ITERS; ++j) {
        const int item = tid + 512 * j;
        const int m = item / (KS / AV), qd = item - m * (KS / AV);
        const bool used = item < A_ITEMS && m0 + m < a.M;
        avo[j] = used ? (unsigned)(((int64_t)(m0 + m) * g.y_cs + AV * qd) * ESZ) : 0xffffffffu;
        alds[j] = m * AP + qd * (AV * 2);
    }
    int lb[NS][2];
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int p = 16 * s + 8 * (lane >> 5) + 4 * h + ((lane & 15) >> 2);
            const int j = p / PP, r = p - j * PP;
            lb[s][h] = j * SLAB + ((r / 3) * 5 + r % 3) * 64 + ((lane >> 4) & 1) * 32 + (lane & 3) * 8;
        }
    int toff[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int tau = min(wave + 8 * j, 26);
        const int dt = tau / 9, dh = (tau / 3) % 3, dw = tau % 3;
        toff[j] = dt * SLAB + (dh * 5 + dw) * 64;
    }
    const bool four = wave < 3;

    unsigned rx[S_ITERS][2][H ? 2 : 4];
    Words4 ra[A_ITERS];
    auto load_x = [&](int b, int k) {                        // planes 16k - 1 .. 16k + 16 of sample b (zeros outside 0 .. T-1)
        const int xbase = (int)(((int64_t)b * g.x_bs + (int64_t)ci0 * g.x_cs + (int64_t)(PS * k) * PP) * ESZ);
#pragma unroll
        for (int i = 0; i < S_ITERS; ++i) {
            const bool outside = (sq[i] < 3 && k == 0) || (sq[i] >= 39 && PS * (k + 1) >= T);
            const unsigned vo = (!sused[i] || outside) ? a.src_bytes : (unsigned)(srel[i] + xbase);
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                if constexpr (H) {
                    const Words2 v = __builtin_bit_cast(Words2, __builtin_amdgcn_raw_buffer_load_b64(rxs, vo, h ? (int)(g.x_cs * 2) : 0, 0));
                    rx[i][h][0] = v.a; rx[i][h][1] = v.b;
                } else {
                    const Words4 v = __builtin_bit_cast(Words4, __builtin_amdgcn_raw_buffer_load_b128(rxs, vo, h ? (int)(g.x_cs * 4) : 0, 0));
                    rx[i][h][0] = v.a; rx[i][h][1] = v.b; rx[i][h][2] = v.c; rx[i][h][3] = v.d;
                }
            }
        }
    };
    auto store_x = [&](int buf) {
        unsigned char* X = smem + buf * XB;
#pragma unroll
        for (int i = 0; i < S_ITERS; ++i) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const unsigned off = (scell[i][e >> 1] >> (16 * (e & 1))) & 0xffffu;
                if (off == 0xffffu) continue;
                unsigned* dst = reinterpret_cast<unsigned*>(X + off);
                if constexpr (H) *dst = (e & 1) ? pair_hi(rx[i][0][e >> 1], rx[i][1][e >> 1]) : pair_lo(rx[i][0][e >> 1], rx[i][1][e >> 1]);
                else *dst = cvt_pk_bf16(__uint_as_float(rx[i][0][e]), __uint_as_float(rx[i][1][e]));
            }
        }
    };
    auto load_dy = [&](int b, int k) {
        const int ybase = (int)(((int64_t)b * g.y_bs + (int64_t)(PS * k) * PP) * ESZ);
#pragma unroll
        for (int j = 0; j < A_ITERS; ++j)
            ra[j] = __builtin_bit_cast(Words4, __builtin_amdgcn_raw_buffer_load_b128(rdy, avo[j], ybase, 0));
    };
    auto store_dy = [&](int buf) {
        unsigned char* A = smem + 2 * XB + buf * AB;
#pragma unroll
        for (int j = 0; j < A_ITERS; ++j) {
            if (A_ITEMS % 512 != 0 && tid + 512 * j >= A_ITEMS) continue;
            if constexpr (H) {
                *reinterpret_cast<Words4*>(A + alds[j]) = ra[j];
            } else {
                Words2 pk;
                pk.a = cvt_pk_bf16(__builtin_bit_cast(float, ra[j].a), __builtin_bit_cast(float, ra[j].b));
                pk.b = cvt_pk_bf16(__builtin_bit_cast(float, ra[j].c), __builtin_bit_cast(float, ra[j].d));
                *reinterpret_cast<Words2*>(A + alds[j]) = pk;
            }
        }
    };

    f32x16 acc[MT][4];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    typedef __attribute__((address_space(3))) unsigned char lds_byte;
    lds_byte* const lds0 = (lds_byte*)smem;

    int sb = q_begin / KT, sk = q_begin - sb * KT;
    if (q_begin < q_end) {
        load_dy(sb, sk);
        load_x(sb, sk);
        __syncthreads();                                     // the zero fill above
        store_dy(0);
        store_x(0);
    }
    for (int q = q_begin; q < q_end; ++q) {
        const int buf = (q - q_begin) & 1;
        __syncthreads();
        const bool more = q + 1 < q_end;
        int nb = sb, nk = sk + 1;
        if (nk == KT) { nk = 0; ++nb; }
        if (more) { load_dy(nb, nk); load_x(nb, nk); }
        const unsigned char* const A = smem + 2 * XB + buf * AB;
        const int xb = buf * XB;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            bf16x8 av[MT];
#pragma unroll
            for (int i = 0; i < MT; ++i)
                av[i] = *reinterpret_cast<const bf16x8*>(A + (i * 32 + (lane & 31)) * AP + (s * 16 + 8 * (lane >> 5)) * 2);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (j == 3 && !four) continue;
                const v4s16 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                    (__attribute__((address_space(3))) v4s16*)(lds0 + (xb + lb[s][0] + toff[j])));
                const v4s16 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                    (__attribute__((address_space(3))) v4s16*)(lds0 + (xb + lb[s][1] + toff[j])));
                const bf16x8 bv = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
#pragma unroll
                for (int i = 0; i < MT; ++i)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av[i], bv, acc[i][j], 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        if (more) { store_dy(buf ^ 1); store_x(buf ^ 1); }
        sb = nb; sk = nk;
    }
    wd3_epilogue<MT, 16>(a, acc, ci0, m0, split, wave, lane, smem);
}

template <int BM, int PW, int PR, bool H>
static int launch_wd3(const WD3Args& d, dim3 grid, hipStream_t st) {
    constexpr int XB = 4 * (PR + 2) * (PW + 2) * 64, AB = BM * (PR * PW * 2 + 16);
    constexpr int lds = XB + 2 * AB;
    return launch_big_lds<conv3_wgrad_direct_kernel<BM, PW, PR, H>>(lds, grid, 512, st, d);
}

template <int BM, bool H>
static int launch_wd6(const WD3Args& d, dim3 grid, hipStream_t st) {
    constexpr int lds = 16 * 4096 + 2 * BM * (144 * 2 + 16);
    return launch_big_lds<conv3_wgrad_planes6_kernel<BM, H>>(lds, grid, 512, st, d);
}

template <int BM, bool H>
static int launch_wd3p(const WD3Args& d, dim3 grid, hipStream_t st) {
    constexpr int lds = 2 * 18 * 25 * 64 + 2 * BM * (144 * 2 + 16);
    return launch_big_lds<conv3_wgrad_planes3_kernel<BM, H>>(lds, grid, 512, st, d);
}

template <bool H = false>
int launch_wgrad_direct(ConvArgs& a, const ConvLaunchShape& sh, void* ws, hipStream_t st) {
    const ConvGeom& g = a.g;
    const bool planes6 = g.Wi == 6, planes3 = g.Wi == 3;
    const int PRr = wgrad_direct_rows(g);      // (tile height, K steps and splits: conv_select.h, wgrad_direct_shape)
    WD3Args d;
    d.HB = g.Hi / PRr;
    d.steps = sh.units;
    d.sps = sh.per_split;
    a.fd = make_conv_fastdiv(g);
    a.src_bytes = (unsigned)gather_extent_bytes(g, MODE_FWD, H ? 2 : 4);
    a.dy_bytes = (unsigned)gather_extent_bytes(g, MODE_DGRAD, H ? 2 : 4);
    if (!set_splits<MODE_WGRAD>(a, sh, ws)) return OTAL_E_UNSUPPORTED;      // 32-bit store offsets
    d.c = a;
    const dim3 grid(sh.grid[0], sh.grid[1], sh.grid[2]);
    int e;
    if (planes3) e = launch_wd3p<32, H>(d, grid, st);
    else if (planes6) e = launch_wd6<32, H>(d, grid, st);
    else if (g.Wi == 24) e = PRr == 8 ? launch_wd3<64, 24, 8, H>(d, grid, st) : launch_wd3<64, 24, 4, H>(d, grid, st);
    else e = launch_wd3<64, 12, 12, H>(d, grid, st);    // whole 12x12 planes: 9 k16 steps per barrier (4 rows: 3 steps, 0.44 -> ms)
    if (e) return e;
    return a.splits > 1 ? launch_splitk_reduce<MODE_WGRAD>(a, st) : 0;
}
