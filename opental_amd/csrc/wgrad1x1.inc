// opental_amd/csrc/wgrad1x1.inc -- included by conv_gemm.hip inside its anonymous namespace.
//
// Weight gradient of the 1x1x1 convolutions of the I3D backbone (Conv3d_2b, the fused / pooled 1x1 branches of every
// Inception module; autograd of AFSD/common/i3d_backbone.py:33-43):  dW[co][ci] = sum over positions dy[co][p] * x[ci][p].
// M = Cout and N = Cin are small (32 .. 832) while K = B * T * H * W is 18 k .. 590 k: the operation is a stream over x and
// dy, and it is only HBM-optimal if each is read ONCE.  The tiled vector kernel cuts M x N into 96..128 x 128 tiles, every
// tile re-reading its operand rows (Mixed_3c: x three times, dy twice -> 2.2 TB/s effective).  Here ONE workgroup holds
// up to 288 x 256 of dW in its accumulators (8 waves x 9 MFMA tiles) and streams a K range: both operands are
// K(position)-contiguous rows, staged with 16-byte loads, bf16 in LDS, fragments by ds_read_b128 -- a plain "NT" GEMM with
// no gather at all.  Split-K slabs, reduced in order by splitk_reduce_kernel.
// H: x and dy are STORED as bf16: a 16-byte load carries eight positions and goes to LDS as it is (half the load
// instructions, no conversion; the operands are the values the fp32-tensor kernel rounds to).
template <int MT, bool H = false>
__global__ __launch_bounds__(512) void wgrad1x1_wide_kernel(const ConvArgs a) {
    constexpr int RA = MT * 32, RB = 256, KS = 32, PITCH = KS * 2 + 16;     // 80-byte rows: conflict-free ds_read_b128
    constexpr int ESZ = H ? 2 : 4, PV = H ? 8 : 4;                           // bytes per element, positions per 16-byte load
    constexpr int QUADS = (RA + RB) * (KS / PV), ITERS = (QUADS + 511) / 512;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];    // [2][(RA + RB) * PITCH]
    constexpr int BUF = (RA + RB) * PITCH;
    const ConvGeom& g = a.g;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const TileId tile = xcd_tile(false);                    // x: 256-column block of Cin, y: row block of Cout, z: split
    const int n0 = tile.x * RB, m0 = tile.y * RA, split = tile.z;
    const int k_begin = split * a.k_per_split, k_end = min(a.K, k_begin + a.k_per_split);
    const int nk = (k_end - k_begin) / KS;
    const auto rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.x), 0, (int)a.src_bytes, 0x00020000);
    const auto rdy = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.dy), 0, (int)a.dy_bytes, 0x00020000);

    // staging items: rows 0 .. RA-1 = dy channels m0 + row, rows RA .. = x channels n0 + row - RA; 8 quads of positions each
    unsigned vo[ITERS];
    int lds_off[ITERS];
    bool isx[ITERS];
#pragma unroll
    for (int i = 0; i < ITERS; ++i) {
        const int item = tid + 512 * i;
        const int row = item / (KS / PV), q = item % (KS / PV);
        isx[i] = row >= RA;
        const int ch = isx[i] ? n0 + row - RA : m0 + row;
        const bool ok = item < QUADS && ch < (isx[i] ? a.N : a.M);
        vo[i] = ok ? (unsigned)(((int64_t)ch * (isx[i] ? g.x_cs : g.y_cs) + q * PV) * ESZ) : 0xffffffffu;
        lds_off[i] = item < QUADS ? row * PITCH + q * (PV * 2) : -1;
    }
    Words4 rr[ITERS];
    auto load = [&](int k0) {                               // a K step never leaves its sample (P % 32 == 0)
        const uint32_t b = fd_div(a.fd.P, (uint32_t)k0);
        const int p = k0 - (int)(b * a.fd.P.d);
        const int sx = (int)(((int64_t)b * g.x_bs + p) * ESZ), sy = (int)(((int64_t)b * g.y_bs + p) * ESZ);
#pragma unroll
        for (int i = 0; i < ITERS; ++i)
            rr[i] = isx[i] ? __builtin_bit_cast(Words4, __builtin_amdgcn_raw_buffer_load_b128(rx, vo[i], sx, 0))
                           : __builtin_bit_cast(Words4, __builtin_amdgcn_raw_buffer_load_b128(rdy, vo[i], sy, 0));
    };
    auto store = [&](int buf) {
        unsigned char* S = smem + buf * BUF;
#pragma unroll
        for (int i = 0; i < ITERS; ++i) {
            if (lds_off[i] < 0) continue;
            if constexpr (H) {
                *reinterpret_cast<Words4*>(S + lds_off[i]) = rr[i];
            } else {
                Words2 pk;
                pk.a = cvt_pk_bf16(__builtin_bit_cast(float, rr[i].a), __builtin_bit_cast(float, rr[i].b));
                pk.b = cvt_pk_bf16(__builtin_bit_cast(float, rr[i].c), __builtin_bit_cast(float, rr[i].d));
                *reinterpret_cast<Words2*>(S + lds_off[i]) = pk;
            }
        }
    };
    f32x16 acc[MT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
    if (nk > 0) { load(k_begin); store(0); }
    __syncthreads();
    const int frag = (lane & 31) * PITCH + (lane >> 5) * 16;
    for (int it = 0; it < nk; ++it) {
        const int buf = it & 1;
        if (it + 1 < nk) load(k_begin + (it + 1) * KS);
        const unsigned char* A = smem + buf * BUF + frag;
        const unsigned char* B = smem + buf * BUF + (RA + wave * 32) * PITCH + frag;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const bf16x8 bv = *reinterpret_cast<const bf16x8*>(B + c * 32);
#pragma unroll
            for (int i = 0; i < MT; ++i) {
                const bf16x8 av = *reinterpret_cast<const bf16x8*>(A + i * 32 * PITCH + c * 32);
                acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, bv, acc[i], 0, 0, 0);
            }
        }
        if (it + 1 < nk) store(buf ^ 1);
        __syncthreads();
    }
    // ---- slab[split][m][n] (or dW itself when there is one split); lanes run along n = ci: coalesced
    const bool slabs = a.splits > 1;
    const auto ro = __builtin_amdgcn_make_buffer_rsrc(slabs ? a.slab : a.out, 0, (int)(slabs ? a.slab_bytes : a.out_bytes), 0x00020000);
    const bool accum = !slabs && (a.flags & EPI_ACCUM);
    const int n = n0 + wave * 32 + (lane & 31);
#pragma unroll
    for (int i = 0; i < MT; ++i) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = m0 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            const unsigned off = (n < a.N && m < a.M) ? (((unsigned)(slabs ? split : 0) * (unsigned)a.M + (unsigned)m) * (unsigned)a.N + (unsigned)n) * 4u : 0xffffffffu;
            float v = acc[i][r];
            if (accum) v += __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(ro, off, 0, 0));
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), ro, off, 0, 0);
        }
    }
}

template <int MT, bool H>
static int launch_w1x1(const ConvArgs& a, dim3 grid, hipStream_t st) {
    constexpr int lds = 2 * (MT * 32 + 256) * 80;
    return launch_big_lds<wgrad1x1_wide_kernel<MT, H>>(lds, grid, 512, st, a);
}

template <bool H = false>
int launch_wgrad1x1_wide(ConvArgs& a, const ConvLaunchShape& sh, void* ws, hipStream_t st) {
    const ConvGeom& g = a.g;
    const int mt = sh.bm / 32;          // row-block height and splits: conv_select.h (wgrad1x1_mt, wgrad1x1_splits)
    a.fd = make_conv_fastdiv(g);
    a.P = conv_out_positions(g);
    a.src_bytes = (unsigned)gather_extent_bytes(g, MODE_FWD, H ? 2 : 4);
    a.dy_bytes = (unsigned)gather_extent_bytes(g, MODE_DGRAD, H ? 2 : 4);
    if (!set_splits<MODE_WGRAD>(a, sh, ws)) return OTAL_E_UNSUPPORTED;
    const dim3 grid(sh.grid[0], sh.grid[1], sh.grid[2]);
    int e;
    switch (mt) {
        case 4: e = launch_w1x1<4, H>(a, grid, st); break;
        case 3: e = launch_w1x1<3, H>(a, grid, st); break;
        default: e = launch_w1x1<2, H>(a, grid, st); break;
    }
    if (e) return e;
    return a.splits > 1 ? launch_splitk_reduce<MODE_WGRAD>(a, st) : 0;
}
