// opental_amd/csrc/conv1a_wgrad.inc -- included by conv_gemm.hip inside its anonymous namespace.
//
// Weight gradient of Conv3d_1a_7x7 (3 -> 64 channels, 7x7x7, stride 2; autograd of AFSD/common/i3d_backbone.py:33-43 for
// the first layer), direct -- the twin of conv1a_direct_fwd_kernel above:
//
//     dW[co][ci][dt][dh][dw] = sum over (b,to,ho,wo)  dy[b][co][to][ho][wo] * x[b][ci][2to+dt-2][2ho+dh-2][2wo+dw-2]
//
// The vector ("pair mode") kernel tiles the 1029 columns in ten 128-column tiles: dy (604 MB) goes through L1 ten
// times and every x window is fetched per column pair -- the single most expensive launch of the step (1.05 ms).
// Here a workgroup owns ONE temporal tap dt and all its 7 x (7 x 3) columns for a range of 2 x 2 x 48 output blocks:
//   * x : the two input planes the block needs for this dt, 9 rows x 104 pixels, staged once as channel-last bf16 pixels
//         {c0, c1, c2, 0} (8 bytes) -- the forward kernel's patch layout, zero borders included;
//   * dy: the block's 64 x 192 values, bf16, position(K)-contiguous -> A fragments by ds_read_b128;
//   * B fragment of kernel row (dt, dh) for 8 consecutive wo: ds_read_b64_tr_b16 over [4 positions][4 pixels x 4 ch]
//     blocks -- position wo starts at pixel 2 wo, its 8 dw taps x 4 channels are 64 contiguous bytes, so each lane quad
//     supplies ONE address (lane constant + compile-time offset) and no gather, mask or shuffle is needed.  Columns with
//     ci = 3 or dw = 7 are computed on zero / foreign pixels and dropped in the epilogue (21 of 32 columns are real).
// Accumulators stay in registers over the whole block range; split-K slabs, reduced in order by splitk_reduce_kernel.
struct W1aArgs {
    ConvArgs c;
    int nblocks, bps;          // 2x2x48 output blocks in all, per split
};

// DYH: dy is STORED as bf16 (written so by the max-pool backward kernel): 16-byte loads carry 8 positions and go to LDS as
// they are -- half the load instructions and no conversion (the values are the ones the fp32 path rounds to).
template <bool DYH>
__global__ __launch_bounds__(256, 2) void conv1a_wgrad_direct_kernel(const W1aArgs d) {
    constexpr int PITCH = C1_PITCH;                         // 104 pixels x 8 bytes
    constexpr int PATCH = 2 * C1_NR * PITCH;                // two planes
    constexpr int AP = 192 * 2 + 16;                        // dy row pitch (conflict-free ds_read_b128)
    __shared__ __attribute__((aligned(16))) unsigned char lds[PATCH + 64 * AP];
    unsigned char* const patch = lds;
    unsigned char* const dyT = lds + PATCH;
    const ConvArgs& a = d.c;
    const ConvGeom& g = a.g;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // the seven taps of one block range read the same dy tiles: logical tiles (dt fastest) are dealt to the XCDs in
    // contiguous ranges, so the seven workgroups run side by side on ONE XCD and dy crosses the fabric once, not 7 times
    // (first version, taps far apart in dispatch order: 4.2 GB of dy re-reads, the kernel ran at 5.8 TB/s -- HBM-bound)
    const TileId tile = xcd_tile(false);
    const int dt = tile.x, split = tile.y;
    const int blk_begin = split * d.bps, blk_end = min(d.nblocks, blk_begin + d.bps);
    const int tiles_h = g.Ho / 2, tiles_t = g.To / 2;
    const int HWo = g.Ho * g.Wo;
    const auto rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.x), 0, (int)a.src_bytes, 0x00020000);
    const auto rdy = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.dy), 0, (int)a.dy_bytes, 0x00020000);

    for (int i = tid; i < PATCH / 16; i += 256) reinterpret_cast<uint4*>(patch)[i] = make_uint4(0u, 0u, 0u, 0u);   // zero side columns stay

    // ---- staging items
    constexpr int X_ITEMS = 2 * C1_NR * 24, X_ITERS = (X_ITEMS + 255) / 256;        // (plane, row, quad of pixels)
    int xrel[X_ITERS], xlds[X_ITERS], xpr[X_ITERS];
#pragma unroll
    for (int i = 0; i < X_ITERS; ++i) {
        const int item = tid + 256 * i;
        const int pl = item / (C1_NR * 24), rem = item - pl * (C1_NR * 24), rr = rem / 24, q = rem - rr * 24;
        xrel[i] = ((2 * pl) * g.Hi + rr) * g.Wi + 4 * q;                             // elements, relative to (ti0, hi0, 0)
        xlds[i] = item < X_ITEMS ? (pl * C1_NR + rr) * PITCH + (4 * q + 2) * 8 : -1;
        xpr[i] = (pl << 8) | rr;
    }
    constexpr int A_ITERS = DYH ? 64 * 24 / 256 : 64 * 48 / 256;    // (co, run of 48 positions, quad [oct] of positions)
    unsigned avo[A_ITERS];
    int alds[A_ITERS];
#pragma unroll
    for (int j = 0; j < A_ITERS; ++j) {
        const int item = tid + 256 * j;
        if constexpr (DYH) {
            const int co = item / 24, rem = item - co * 24, run = rem / 6, o = rem - run * 6;
            avo[j] = co < a.M ? (unsigned)(((int64_t)co * g.y_cs + (run >> 1) * HWo + (run & 1) * g.Wo + 8 * o) * 2) : 0xffffffffu;
            alds[j] = co * AP + (run * 48 + 8 * o) * 2;
        } else {
            const int co = item / 48, rem = item - co * 48, run = rem / 12, q = rem - run * 12;
            avo[j] = co < a.M ? (unsigned)(((int64_t)co * g.y_cs + (run >> 1) * HWo + (run & 1) * g.Wo + 4 * q) * 4) : 0xffffffffu;
            alds[j] = co * AP + (run * 48 + 4 * q) * 2;
        }
    }
    // ---- fragment addresses.  K position p = 16 s + 8 (lane >> 5) + 4 h + ((lane & 15) >> 2); s = 3 * (tl * 2 + hl) + wl0 / 16
    // this wave: kernel rows dh0 .. dh0 + 3 (group 0) or 4 .. 6 (group 1), BOTH 32-row tiles of the output channels, and every
    // SECOND k16 step of a block (khalf); the two halves' sums meet in LDS after the block loop.  (First version: one m-tile x
    // rows dh0, dh0 + 2, .. per wave, every step -- an x fragment, two transposing 8-byte reads per lane, fed ONE MFMA: 1.29 KB
    // of LDS reads per MFMA with the LDS pipe the busiest unit of the kernel.  Second: rows 2 wave, 2 wave + 1 and both m-tiles
    // per wave, every step -- all four waves read the same dy fragments: 1.07 KB.  Here two waves share a step: 0.79 KB.)
    const int grp = wave & 1, khalf = wave >> 1;
    const int dh0 = 4 * grp;
    const int lanex = (2 * (8 * (lane >> 5) + ((lane & 15) >> 2)) + 4 * ((lane >> 4) & 1) + (lane & 3)) * 8;
    const unsigned char* const arow = dyT + (lane & 31) * AP + (lane >> 5) * 16;
    typedef __attribute__((address_space(3))) unsigned char lds_byte;
    lds_byte* const xl = (lds_byte*)patch + lanex + dh0 * PITCH;

    int xoffs[6], aoffs[6];
#pragma unroll
    for (int s2 = 0; s2 < 6; ++s2) {
        const int s = 2 * s2 + khalf;
        const int run = s / 3, w16 = s - run * 3, tl = run >> 1, hl = run & 1;
        xoffs[s2] = __builtin_amdgcn_readfirstlane((tl * C1_NR + 2 * hl) * PITCH + (2 * 16 * w16) * 8);
        aoffs[s2] = __builtin_amdgcn_readfirstlane(s * 32);
    }
    f32x16 acc[2][4];                                       // [m-tile][row dh0 + j]
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // Software pipeline through registers: the loads of block i+1 are in flight while block i is multiplied.
    float4 xv[X_ITERS][3];
    Words4 ra[A_ITERS];
    auto load = [&](int blk) {
        int bid = blk;
        const int th = bid % tiles_h; bid /= tiles_h;
        const int tt0 = bid % tiles_t;
        const int b = bid / tiles_t;
        const int to0 = tt0 * 2, ho0 = th * 2;
        const int ti0 = 2 * to0 - g.pt + dt, hi0 = 2 * ho0 - g.ph;
        const int64_t xb0 = (int64_t)b * g.x_bs + ((int64_t)ti0 * g.Hi + hi0) * g.Wi;
#pragma unroll
        for (int i = 0; i < X_ITERS; ++i) {
            const int pl = xpr[i] >> 8, rr = xpr[i] & 255;
            const bool ok = xlds[i] >= 0 && (unsigned)(ti0 + 2 * pl) < (unsigned)g.Ti && (unsigned)(hi0 + rr) < (unsigned)g.Hi;
            const unsigned vo = ok ? (unsigned)((xb0 + xrel[i]) * 4) : 0xffffffffu;
#pragma unroll
            for (int ci = 0; ci < 3; ++ci) {
                const Words4 v = __builtin_bit_cast(Words4, __builtin_amdgcn_raw_buffer_load_b128(rx, vo, (int)(ci * g.x_cs * 4), 0));
                xv[i][ci] = make_float4(__uint_as_float(v.a), __uint_as_float(v.b), __uint_as_float(v.c), __uint_as_float(v.d));
            }
        }
        const int ybase = (int)(((int64_t)b * g.y_bs + (int64_t)to0 * HWo + ho0 * g.Wo) * (DYH ? 2 : 4));
#pragma unroll
        for (int j = 0; j < A_ITERS; ++j)
            ra[j] = __builtin_bit_cast(Words4, __builtin_amdgcn_raw_buffer_load_b128(rdy, avo[j], ybase, 0));
    };
    if (blk_begin < blk_end) load(blk_begin);
    for (int blk = blk_begin; blk < blk_end; ++blk) {
        __syncthreads();                                    // the previous block's operand reads are done
#pragma unroll
        for (int i = 0; i < X_ITERS; ++i) {
            if (xlds[i] < 0) continue;
            uint2* dst = reinterpret_cast<uint2*>(patch + xlds[i]);
            dst[0] = make_uint2(cvt_pk_bf16(xv[i][0].x, xv[i][1].x), cvt_pk_bf16(xv[i][2].x, 0.f));
            dst[1] = make_uint2(cvt_pk_bf16(xv[i][0].y, xv[i][1].y), cvt_pk_bf16(xv[i][2].y, 0.f));
            dst[2] = make_uint2(cvt_pk_bf16(xv[i][0].z, xv[i][1].z), cvt_pk_bf16(xv[i][2].z, 0.f));
            dst[3] = make_uint2(cvt_pk_bf16(xv[i][0].w, xv[i][1].w), cvt_pk_bf16(xv[i][2].w, 0.f));
        }
#pragma unroll
        for (int j = 0; j < A_ITERS; ++j) {
            if constexpr (DYH) {
                *reinterpret_cast<Words4*>(dyT + alds[j]) = ra[j];
            } else {
                Words2 pk;
                pk.a = cvt_pk_bf16(__builtin_bit_cast(float, ra[j].a), __builtin_bit_cast(float, ra[j].b));
                pk.b = cvt_pk_bf16(__builtin_bit_cast(float, ra[j].c), __builtin_bit_cast(float, ra[j].d));
                *reinterpret_cast<Words2*>(dyT + alds[j]) = pk;
            }
        }
        __syncthreads();
        if (blk + 1 < blk_end) load(blk + 1);
        // ---- 12 k16 steps: s = 3 * run + w16, run = tl * 2 + hl; this wave takes s = 2 s2 + khalf (offsets: wave-uniform scalars)
#pragma unroll
        for (int s2 = 0; s2 < 6; ++s2) {
            const bf16x8 av0 = *reinterpret_cast<const bf16x8*>(arow + aoffs[s2]);
            const bf16x8 av1 = *reinterpret_cast<const bf16x8*>(arow + 32 * AP + aoffs[s2]);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (j == 3 && grp) continue;
                const v4s16 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                    (__attribute__((address_space(3))) v4s16*)(xl + xoffs[s2] + j * PITCH));
                const v4s16 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                    (__attribute__((address_space(3))) v4s16*)(xl + xoffs[s2] + j * PITCH + 64));
                const bf16x8 bv = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                acc[0][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av0, bv, acc[0][j], 0, 0, 0);
                acc[1][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av1, bv, acc[1][j], 0, 0, 0);
            }
        }
    }

    // ---- the odd-step waves hand their sums to the even-step ones, one 32-row tile at a time (32 KB of the operand buffers)
    float* const xch = reinterpret_cast<float*>(lds);
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        __syncthreads();
        if (khalf) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) xch[((grp * 4 + j) * 16 + r) * 64 + lane] = acc[mt][j][r];
        }
        __syncthreads();
        if (!khalf) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[mt][j][r] += xch[((grp * 4 + j) * 16 + r) * 64 + lane];
        }
    }
    if (khalf) return;

    // ---- epilogue: column n of tile (dt, dh) = (dw = n >> 2, ci = n & 3); dW[co][ci][dt][dh][dw]
    const bool slabs = a.splits > 1;
    const auto ro = __builtin_amdgcn_make_buffer_rsrc(slabs ? a.slab : a.out, 0, (int)(slabs ? a.slab_bytes : a.out_bytes), 0x00020000);
    const bool accum = !slabs && (a.flags & EPI_ACCUM);
    const int nn = lane & 31, dw = nn >> 2, ci = nn & 3;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (j == 3 && grp) continue;
        const int dh = dh0 + j;
        const unsigned col = (unsigned)(ci * 343 + dt * 49 + dh * 7 + dw);
        const bool okn = ci < 3 && dw < 7;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                const unsigned vo = (okn && m < a.M) ? (((unsigned)(slabs ? split : 0) * (unsigned)a.M + (unsigned)m) * (unsigned)a.N + col) * 4u : 0xffffffffu;
                float v = acc[mt][j][r];
                if (accum) v += __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(ro, vo, 0, 0));
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), ro, vo, 0, 0);
            }
    }
}

int launch_conv1a_wgrad(ConvArgs& a, const ConvLaunchShape& sh, void* ws, hipStream_t st) {
    const ConvGeom& g = a.g;
    W1aArgs d;
    d.nblocks = sh.units;           // 2 x 2 x 48 output blocks, sh.per_split per split (conv_select.h)
    d.bps = sh.per_split;
    a.src_bytes = (unsigned)gather_extent_bytes(g, MODE_FWD);
    a.dy_bytes = (unsigned)(gather_extent_bytes(g, MODE_DGRAD) >> (a.half ? 1 : 0));
    a.flags &= ~EPI_NPAD8;
    if (!set_splits<MODE_WGRAD>(a, sh, ws)) return OTAL_E_UNSUPPORTED;
    d.c = a;
    if (a.half) hipLaunchKernelGGL(conv1a_wgrad_direct_kernel<true>, dim3(7, a.splits), dim3(256), 0, st, d);
    else hipLaunchKernelGGL(conv1a_wgrad_direct_kernel<false>, dim3(7, a.splits), dim3(256), 0, st, d);
    if (int e = otal_launch_status()) return e;
    return a.splits > 1 ? launch_splitk_reduce<MODE_WGRAD>(a, st) : 0;
}
