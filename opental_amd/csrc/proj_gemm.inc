// opental_amd/csrc/proj_gemm.inc -- included by conv_gemm.hip inside its anonymous namespace.
//
// Forward of the pyramid projection Unit3D [1,6,6] 832 -> 512 (spatial_valid: the kernel covers the whole 6x6 plane;
// AFSD/thumos14/BDNet.py:129-155, layers.py:107-175): y[b][co][t] = sum over (ci, h, w) W[co][ci][h][w] * x[b][ci][t][h][w].
// A GEMM with M = 512, N = B * 64, K = 29 952 whose operands are BOTH K-contiguous: a weight row is 29 952 consecutive floats
// and, for one (sample, t), the 36 values of a channel are consecutive.  The tiled gather kernel fetched B along N (one
// 4-byte element per lane, 144 bytes apart: 64 cache lines per load instruction) and ran at 60 TFLOP/s / 236 GB/s on
// this 61 MB-weight layer.  Here both tiles are staged with 16-byte loads along K -- fp32 weights straight from the
// parameter arena (no packed copy, no prologue), converted to bf16 on the way into LDS -- in K steps of four input
// channels (144 k); split-K over channel ranges, slabs reduced (+ bias) in order by splitk_reduce_kernel.
constexpr int PJ_KS = 4 * PJ_HW, PJ_PITCH = PJ_KS * 2 + 16;     // (PJ_HW, the 36 positions of a plane: conv_select.h)

__global__ __launch_bounds__(256) void proj_fwd_kernel(const ConvArgs a, int ci_per_split) {
    constexpr int Q = PJ_KS / 4;                            // 16-byte quads per row and K step
    constexpr int ITERS = 64 * Q / 256;                     // per operand and thread
    static_assert(64 * Q % 256 == 0, "tiling");
    __shared__ __attribute__((aligned(16))) unsigned char sA[2][64 * PJ_PITCH];
    __shared__ __attribute__((aligned(16))) unsigned char sB[2][64 * PJ_PITCH];
    const ConvGeom& g = a.g;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int T = g.To, nblk = (T + 63) / 64;
    // grid = (splits, m tiles, n blocks): workgroups go to the XCDs round-robin by linear index, so with the SPLIT fastest the 64
    // workgroups of one channel range (8 splits at b = 8) sit on ONE XCD and walk their 7.7 MB slices of W and x in step: each
    // slice crosses the fabric once and is shared through that XCD's L2.  With the m tile fastest (the first version) an XCD held one
    // m tile of every split: the x slices were fetched by all eight XCDs (0.5 GB instead of 61 MB).
    const int m0 = blockIdx.y * 64;
    const int b = blockIdx.z / nblk, t0 = (blockIdx.z - b * nblk) * 64;
    const int split = blockIdx.x;
    const int ci_begin = split * ci_per_split, ci_end = min(g.Cin, ci_begin + ci_per_split);
    const int nsteps = (ci_end - ci_begin) / 4;
    const int K = g.Cin * PJ_HW;
    const auto rw = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.w), 0, (int)a.wp_bytes, 0x00020000);
    const auto rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.x), 0, (int)a.src_bytes, 0x00020000);

    unsigned avo[ITERS], bvo[ITERS];
    int lds_off[ITERS];
#pragma unroll
    for (int i = 0; i < ITERS; ++i) {
        const int item = tid + 256 * i;
        const int row = item / Q, q = item - row * Q;       // q: quad inside the 144-wide K step
        const int cil = q / (PJ_HW / 4), hq = q - cil * (PJ_HW / 4);
        avo[i] = m0 + row < a.M ? (unsigned)(((int64_t)(m0 + row) * K + q * 4) * 4) : 0xffffffffu;
        bvo[i] = t0 + row < T ? (unsigned)(((int64_t)b * g.x_bs + (int64_t)cil * g.x_cs + (int64_t)(t0 + row) * PJ_HW + hq * 4) * 4) : 0xffffffffu;
        lds_off[i] = row * PJ_PITCH + q * 8;
    }
    Words4 ra[ITERS], rb[ITERS];
    auto load = [&](int step) {
        const int ci = ci_begin + 4 * step;
        const int ao = ci * PJ_HW * 4, bo = (int)((int64_t)ci * g.x_cs * 4);
#pragma unroll
        for (int i = 0; i < ITERS; ++i) {
            ra[i] = __builtin_bit_cast(Words4, __builtin_amdgcn_raw_buffer_load_b128(rw, avo[i], ao, 0));
            rb[i] = __builtin_bit_cast(Words4, __builtin_amdgcn_raw_buffer_load_b128(rx, bvo[i], bo, 0));
        }
    };
    auto store = [&](int buf) {
#pragma unroll
        for (int i = 0; i < ITERS; ++i) {
            Words2 pa, pb;
            pa.a = cvt_pk_bf16(__builtin_bit_cast(float, ra[i].a), __builtin_bit_cast(float, ra[i].b));
            pa.b = cvt_pk_bf16(__builtin_bit_cast(float, ra[i].c), __builtin_bit_cast(float, ra[i].d));
            pb.a = cvt_pk_bf16(__builtin_bit_cast(float, rb[i].a), __builtin_bit_cast(float, rb[i].b));
            pb.b = cvt_pk_bf16(__builtin_bit_cast(float, rb[i].c), __builtin_bit_cast(float, rb[i].d));
            *reinterpret_cast<Words2*>(sA[buf] + lds_off[i]) = pa;
            *reinterpret_cast<Words2*>(sB[buf] + lds_off[i]) = pb;
        }
    };
    const int mt = wave & 1, nt = wave >> 1;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    if (nsteps > 0) { load(0); store(0); }
    __syncthreads();
    for (int s = 0; s < nsteps; ++s) {
        const int buf = s & 1;
        if (s + 1 < nsteps) load(s + 1);
        const unsigned char* ar = sA[buf] + (mt * 32 + (lane & 31)) * PJ_PITCH + (lane >> 5) * 16;
        const unsigned char* br = sB[buf] + (nt * 32 + (lane & 31)) * PJ_PITCH + (lane >> 5) * 16;
#pragma unroll
        for (int k = 0; k < PJ_KS / 16; ++k) {
            const bf16x8 av = *reinterpret_cast<const bf16x8*>(ar + k * 32);
            const bf16x8 bv = *reinterpret_cast<const bf16x8*>(br + k * 32);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, bv, acc, 0, 0, 0);
        }
        if (s + 1 < nsteps) store(buf ^ 1);
        __syncthreads();
    }
    // ---- partial sums to slab[split][m][n], n = b * T + t (or the final values when there is one split)
    const int t = t0 + nt * 32 + (lane & 31);
    const bool slabs = a.splits > 1;
    const auto ro = __builtin_amdgcn_make_buffer_rsrc(slabs ? a.slab : a.out, 0, (int)(slabs ? a.slab_bytes : a.out_bytes), 0x00020000);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int m = m0 + mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        const bool ok = t < T && m < a.M;
        float v = acc[r];
        unsigned vo;
        if (slabs) {
            vo = ok ? (((unsigned)split * (unsigned)a.M + (unsigned)m) * (unsigned)a.N + (unsigned)(b * T + t)) * 4u : 0xffffffffu;
        } else {
            const int mc = m < a.M ? m : 0;
            if (a.scale) v *= a.scale[mc];
            if (a.shift) v += a.shift[mc];
            if (a.flags & EPI_RELU) v = fmaxf(v, 0.f);
            vo = ok ? (unsigned)(((int64_t)b * g.y_bs + (int64_t)m * g.y_cs + t) * 4) : 0xffffffffu;
        }
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), ro, vo, 0, 0);
    }
}

int launch_proj_fwd(ConvArgs& a, const ConvLaunchShape& sh, void* ws, hipStream_t st) {
    const ConvGeom& g = a.g;
    a.fd = make_conv_fastdiv(g);
    a.src_bytes = (unsigned)gather_extent_bytes(g, MODE_FWD);
    a.wp_bytes = (unsigned)(4 * (int64_t)g.Cout * g.Cin * PJ_HW);
    if (!set_splits<MODE_FWD>(a, sh, ws)) return OTAL_E_UNSUPPORTED;    // (the channels per split: conv_select.h, proj_fwd_splits)
    a.k_per_split = 0;
    hipLaunchKernelGGL(proj_fwd_kernel, dim3(sh.grid[0], sh.grid[1], sh.grid[2]), dim3(256), 0, st, a, sh.per_split);
    if (int e = otal_launch_status()) return e;
    if (a.splits > 1) return launch_splitk_reduce<MODE_FWD>(a, st);
    return 0;
}

// ---- Weight gradient of the pyramid projections (Unit3D [1,6,6] 832 -> 512 on Mixed_4f and [1,3,3] 1024 -> 512 on Mixed_5c,
// spatial_valid; autograd of AFSD/thumos14/BDNet.py:129-155,:310-319):
//
//     dW[co][ci][hw] = sum over (b, t)  dc[b][co][t] * x[b][ci][t][hw]
//
// A GEMM with M = 512, N = Cin * HW (29 952 / 9 216) and K = B * T (512 / 256 at b = 8): SHORT in K and wide in N -- the
// 61 MB gradient is written once, x (as large) is read once, 1 MB of dc.  The tiled gather kernel that had it
// (conv_gemm_kernel<128,128,...>: one 4-byte element per lane and k, split-K slabs + a reduce launch) ran at 0.113 + 0.054 ms
// -- 138 / 45 TFLOP/s -- on the WEIGHT-GRADIENT lane, which is the critical path of the backward pass.  Here:
//   * no split-K: a workgroup owns a 128 x 128 tile of dW and walks the whole K in steps of 32 frames; the result goes
//     straight to the gradient (arena slot), no slabs, no reduce;
//   * both operands are staged along their contiguous direction -- dc rows are 32 consecutive frames (128 bytes), and for
//     one channel the [frame][hw] block of x is contiguous, so a quad of four columns at one frame is ONE 16-byte load
//     (HW % 4 == 0: the 6 x 6 projection); frames are paired so a lane writes bf16 PAIRS along K into the [column][k] tile
//     the MFMA fragments read as 16-byte pieces.  The 3 x 3 projection (HW = 9: quads straddle channels) loads per element;
//   * the four row tiles of one column tile are dealt to ONE XCD (workgroups go to the XCDs round-robin): the x tile is
//     fetched into that L2 once.
constexpr int PW_PITCH = PW_KS * 2 + 16;        // LDS row pitch (bytes) of both tiles (PW_KS frames per K step)

template <bool QUAD>
__global__ __launch_bounds__(256) void proj_wgrad_kernel(const ConvArgs a, int HW, int tilesM, int tilesN) {
    __shared__ __attribute__((aligned(16))) unsigned char sA[2][128 * PW_PITCH];
    __shared__ __attribute__((aligned(16))) unsigned char sB[2][128 * PW_PITCH];
    const ConvGeom& g = a.g;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // tile map: XCD x = linear % 8 takes column tiles x, x + 8, ...; consecutive workgroups of an XCD = the row tiles of one
    // column tile
    int mt, nt;
    {
        const int lin = blockIdx.x, xcd = lin & 7, idx = lin >> 3;
        const int ncols8 = (tilesN + 7) >> 3;               // column tiles per XCD (the grid is padded to 8 * ncols8 * tilesM)
        mt = idx % tilesM;
        nt = (idx / tilesM) * 8 + xcd;
        if (idx / tilesM >= ncols8 || nt >= tilesN) return;
    }
    const int m0 = mt * 128, n0 = nt * 128;
    const int T = g.To;
    const int spb = T / PW_KS;                              // K steps per sample
    const int nsteps = g.B * spb;
    const auto rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.x), 0, (int)a.src_bytes, 0x00020000);
    const auto rdy = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.dy), 0, (int)a.dy_bytes, 0x00020000);

    // ---- staging items.  A: (row, quad of frames): 128 x 8 = 1024 -> 4 per thread.
    unsigned avo[4];
    int alds[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int item = tid + 256 * i, row = item >> 3, q = item & 7;
        avo[i] = m0 + row < a.M ? (unsigned)(((int64_t)(m0 + row) * g.y_cs + 4 * q) * 4) : 0xffffffffu;
        alds[i] = row * PW_PITCH + q * 8;
    }
    // B: QUAD: (frame pair, column quad): 16 x 32 = 512 -> 2 per thread, two 16-byte loads each;
    //    else: (frame pair, column): 16 x 128 = 2048 -> 8 per thread, two 4-byte loads each
    constexpr int BI = QUAD ? 2 : 8;
    unsigned bvo[BI];
    int blds[BI];
#pragma unroll
    for (int i = 0; i < BI; ++i) {
        const int item = tid + 256 * i;
        int tp, col;
        if (QUAD) { tp = item >> 5; col = (item & 31) * 4; } else { tp = item >> 7; col = item & 127; }
        const int n = n0 + col;
        const int ci = n / HW, hw = n - ci * HW;
        bvo[i] = n < a.N ? (unsigned)(((int64_t)ci * g.x_cs + (int64_t)(2 * tp) * HW + hw) * 4) : 0xffffffffu;
        blds[i] = col * PW_PITCH + tp * 4;
    }
    Words4 ra[4];
    Words4 rb[BI][2];
    auto load = [&](int step) {
        const int b = step / spb, t0 = (step - b * spb) * PW_KS;
        const int ao = (int)(((int64_t)b * g.y_bs + t0) * 4);
        const int bo = (int)(((int64_t)b * g.x_bs + (int64_t)t0 * HW) * 4);
#pragma unroll
        for (int i = 0; i < 4; ++i) ra[i] = __builtin_bit_cast(Words4, __builtin_amdgcn_raw_buffer_load_b128(rdy, avo[i], ao, 0));
#pragma unroll
        for (int i = 0; i < BI; ++i)
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                if (QUAD) {
                    rb[i][e] = __builtin_bit_cast(Words4, __builtin_amdgcn_raw_buffer_load_b128(rx, bvo[i], bo + e * HW * 4, 0));
                } else {
                    rb[i][e].a = __builtin_amdgcn_raw_buffer_load_b32(rx, bvo[i], bo + e * HW * 4, 0);
                }
            }
    };
    auto store = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            Words2 p;
            p.a = cvt_pk_bf16(__builtin_bit_cast(float, ra[i].a), __builtin_bit_cast(float, ra[i].b));
            p.b = cvt_pk_bf16(__builtin_bit_cast(float, ra[i].c), __builtin_bit_cast(float, ra[i].d));
            *reinterpret_cast<Words2*>(sA[buf] + alds[i]) = p;
        }
#pragma unroll
        for (int i = 0; i < BI; ++i) {
            unsigned char* d = sB[buf] + blds[i];
            *reinterpret_cast<unsigned*>(d) = cvt_pk_bf16(__builtin_bit_cast(float, rb[i][0].a), __builtin_bit_cast(float, rb[i][1].a));
            if (QUAD) {
                *reinterpret_cast<unsigned*>(d + PW_PITCH) = cvt_pk_bf16(__builtin_bit_cast(float, rb[i][0].b), __builtin_bit_cast(float, rb[i][1].b));
                *reinterpret_cast<unsigned*>(d + 2 * PW_PITCH) = cvt_pk_bf16(__builtin_bit_cast(float, rb[i][0].c), __builtin_bit_cast(float, rb[i][1].c));
                *reinterpret_cast<unsigned*>(d + 3 * PW_PITCH) = cvt_pk_bf16(__builtin_bit_cast(float, rb[i][0].d), __builtin_bit_cast(float, rb[i][1].d));
            }
        }
    };
    const int wm = wave & 1, wn = wave >> 1;                // this wave: rows [64 wm, +64), columns [64 wn, +64)
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    load(0);
    store(0);
    __syncthreads();
    for (int s = 0; s < nsteps; ++s) {
        const int buf = s & 1;
        if (s + 1 < nsteps) load(s + 1);
        const unsigned char* ar = sA[buf] + (wm * 64 + (lane & 31)) * PW_PITCH + (lane >> 5) * 16;
        const unsigned char* br = sB[buf] + (wn * 64 + (lane & 31)) * PW_PITCH + (lane >> 5) * 16;
#pragma unroll
        for (int k = 0; k < PW_KS / 16; ++k) {
            const bf16x8 a0 = *reinterpret_cast<const bf16x8*>(ar + k * 32);
            const bf16x8 a1 = *reinterpret_cast<const bf16x8*>(ar + 32 * PW_PITCH + k * 32);
            const bf16x8 b0 = *reinterpret_cast<const bf16x8*>(br + k * 32);
            const bf16x8 b1 = *reinterpret_cast<const bf16x8*>(br + 32 * PW_PITCH + k * 32);
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b1, acc[1][1], 0, 0, 0);
        }
        if (s + 1 < nsteps) store(buf ^ 1);
        __syncthreads();
    }
    // ---- dW[m][n] (+)= acc: rows of 32 consecutive columns per store instruction
    const auto ro = __builtin_amdgcn_make_buffer_rsrc(a.out, 0, (int)a.out_bytes, 0x00020000);
    const bool accum = (a.flags & EPI_ACCUM) != 0;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int n = n0 + wn * 64 + 32 * j + (lane & 31);
            unsigned vo[16];
            float v[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + wm * 64 + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                vo[r] = (m < a.M && n < a.N) ? (unsigned)(((int64_t)m * a.N + n) * 4) : 0xffffffffu;
                v[r] = acc[i][j][r];
            }
            if (accum) {
                float old[16];
#pragma unroll
                for (int r = 0; r < 16; ++r) old[r] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(ro, vo[r], 0, 0));
#pragma unroll
                for (int r = 0; r < 16; ++r) v[r] += old[r];
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v[r]), ro, vo[r], 0, 0);
        }
}

int launch_proj_wgrad(ConvArgs& a, const ConvLaunchShape& sh, hipStream_t st) {
    const ConvGeom& g = a.g;
    const int HW = g.Hi * g.Wi;
    a.src_bytes = (unsigned)gather_extent_bytes(g, MODE_FWD);
    a.dy_bytes = (unsigned)gather_extent_bytes(g, MODE_DGRAD);
    if (!set_splits<MODE_WGRAD>(a, sh, nullptr)) return OTAL_E_UNSUPPORTED;
    const int tilesM = sh.tm, tilesN = sh.tn;
    const dim3 grid((unsigned)sh.grid[0]);
    if (HW % 4 == 0) hipLaunchKernelGGL(proj_wgrad_kernel<true>, grid, dim3(256), 0, st, a, HW, tilesM, tilesN);
    else hipLaunchKernelGGL(proj_wgrad_kernel<false>, grid, dim3(256), 0, st, a, HW, tilesM, tilesN);
    return otal_launch_status();
}
