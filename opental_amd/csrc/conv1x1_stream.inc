// opental_amd/csrc/conv1x1_stream.inc -- included by conv_gemm.hip inside its anonymous namespace (part 1: bf16-stored tensors).
//
// The 1x1x1 convolutions of the I3D backbone between Conv3d_2b and Mixed_4f on bf16-STORED tensors, forward and data
// gradient (AFSD/common/i3d_backbone.py:33-43 Unit3D with kernel_shape [1,1,1]; the three 1x1 branches b1a | b2a | b0 of an
// InceptionModule, :90-121, run as one fused layer, and b3b behind the branch pool).  Per sample a plain GEMM
//
//     out[m][p] = epilogue( sum_k  W[m][k] * src[k][p] ),     p = position of the sample (T*H*W, contiguous), k = channel
//
// with M, K a few hundred and 10^4 .. 10^5 positions: 2 x the bytes of src and out in FLOPs per byte -- an HBM stream.  The
// chunked kernel (conv_gemm_bf16c_kernel) treats it like any gathered convolution: one 128-position tile per workgroup, 6-17
// K steps between a cold first load and a transposing epilogue, a v_perm transposition of every loaded value on its way to
// LDS, split-K + a reduce launch where the grid is small.  Its workgroups live for a few microseconds and spend them on
// latencies: 2.3 ms per step over 57 launches at 3.5-4 TB/s (DESIGN 4.5).  This kernel is built for the stream instead:
//
//   * PERSISTENT workgroups walk over position tiles; the (tile, K chunk) sequence is ONE software pipeline -- the loads of
//     item i+2 are in flight (registers) while item i is multiplied and item i+1 is written to LDS, across tile boundaries,
//     so a workgroup pays the cold-load latency once per launch, not once per tile;
//   * src rows go to LDS AS THEY ARE ([k][position], 16-byte pieces, row pitch = 64 (mod 256) bytes): the MFMA operand that
//     wants eight consecutive k per lane is read with ds_read_b64_tr_b16 (hardware transpose) -- no v_perm, no conversion;
//   * the roles of the operands are swapped, acc[position][channel] = src^T W^T: a lane then holds FOUR CONSECUTIVE POSITIONS
//     of one channel per accumulator quad, the per-channel epilogue constants are per-LANE registers, and the bf16 results
//     go through a per-wave LDS patch as 8-byte writes and leave as 16-byte pieces in 128 / 64-byte runs -- no workgroup
//     barrier in the epilogue, the other waves keep multiplying;
//   * the weights are the [Mpad][Kp] bf16 pack the chunk path's (persistent) prologue already builds; a K chunk of them
//     (32 k x all rows) is staged next to the src chunk, once per workgroup and chunk;
//   * no split-K, no reduce launch: every workgroup owns whole tiles.  (Where the chunked kernel split K the fp32 sums
//     associate differently: results agree to fp32 rounding before the bf16 store, not bit for bit -- tests/test_half_chain_gpu.py.)
//
// Tile: 128 * NW positions x 32 * MT channels, four waves, wave w = positions [32 NW w, 32 NW (w+1)); MT * NW <= 8 MFMA tiles
// per wave (128 accumulator registers: two workgroups per CU).  Layers with more than 32 * MT channels run as `msplit` row
// groups: sibling workgroups of one tile sit on the same XCD (grid stride a multiple of 8) and the second one finds src in L2.
typedef Words2 __attribute__((may_alias)) Words2A;
typedef Words4 __attribute__((may_alias)) Words4A;
struct S1Args {
    const unsigned short* src;      // bf16: FWD x, DGRAD dy
    const unsigned short* wp;       // bf16 [Mpad][Kp], zero padded (chunk-path pack; DGRAD: the packed transpose)
    unsigned short* out;            // bf16: FWD y, DGRAD dx
    const unsigned short* mask;     // DGRAD: bf16 activation in dx's layout (ReLU mask), or null
    const float* s0;                // FWD: folded-BN scale per row (null: 1); DGRAD: the producer's BN scale (null: 1)
    const float* s1;                // FWD: shift per row (null: 0)
    const float* zero;              // 16 bytes of zeros in device memory: what a row outside K / Mpad reads
    long long src_bs, src_cs, out_bs, out_cs;      // strides in elements
    unsigned out_bytes;             // extent of out / mask (buffer descriptor of the epilogue)
    int M, Mpad, K, Kp, P;
    int tps, tiles;                 // position tiles per sample, in all
    int wgs;                        // persistent workgroups per row group (a multiple of 8)
    int relu;
};

// one LDS-DMA instruction: lane l's 16 bytes at `gsrc` land at LDS byte lds_dst + 16 l.  Not a load hipcc knows about: no
// register destination, no entry in its s_waitcnt bookkeeping -- completion is counted by hand (dma_wait) before a barrier.
__device__ __forceinline__ void dma16(const void* gsrc, unsigned lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
}
template <int N>
__device__ __forceinline__ void dma_wait() { asm volatile("s_waitcnt vmcnt(%0)" :: "n"(N) : "memory"); }

template <int MT, int NW, int MODE>
__global__ __launch_bounds__(256, 2) void conv1x1_stream_kernel(const S1Args a) {
    static_assert(MT * NW <= 8 && (MT & 1) == 0 && MT <= 6, "accumulator budget / weight blocks per wave / LDS ring");
    constexpr int BN = 128 * NW, KC = 32, RING = 3;
    // src stage: [row quad kq][32-position segment][row of the quad][64 B] -- the four rows a transposing read gathers are 256
    // contiguous bytes (all 64 banks once); a DMA block of 1 KB = four segments of one row quad.
    constexpr int XS = KC * BN * 2, XQ = BN * 8;     // bytes per stage / per row quad
    // weight stage: 64-byte rows (32 k), the four 16-byte pieces of a row XOR-swizzled by (row >> 2) & 3: the lane groups of
    // ds_read_b128 then hit 16 distinct bank quads; a DMA block = 16 rows.
    constexpr int WS = MT * 32 * 64, STAGE = XS + WS;
    constexpr int EP = 32 * NW * 2 + 16;             // epilogue patch: bytes per channel row
    constexpr int XB = 2 * NW, WB = MT / 2;          // DMA blocks per wave and item
    constexpr int L = XB + WB;                       // DMA instructions per wave and item
    __shared__ __attribute__((aligned(1024))) unsigned char smem[RING * STAGE + 4 * 32 * EP];
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    typedef __attribute__((address_space(3))) unsigned char lds_byte;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int mg = blockIdx.x / a.wgs, slot = blockIdx.x - mg * a.wgs;
    const int m_base = mg * (MT * 32);
    const int NC = a.Kp / KC;
    const int my_tiles = slot < a.tiles ? (a.tiles - slot + a.wgs - 1) / a.wgs : 0;
    const int items = my_tiles * NC;
    if (items == 0) return;

    const auto ro = __builtin_amdgcn_make_buffer_rsrc(a.out, 0, (int)a.out_bytes, 0x00020000);
    const auto rm = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned short*>(MODE == MODE_DGRAD && a.mask ? a.mask : a.out), 0,
                                                      (int)a.out_bytes, 0x00020000);
    constexpr unsigned OOB = 0x80000000u;           // + any soffset stays out of range (the check does not wrap)

    // ---- epilogue constants: this lane's channel of every row tile (ordinary loads: drained before the first DMA, so that
    // hipcc's own wait counts -- which do not see the DMA -- are never relied upon for them)
    float e0[MT], e1[MT];
#pragma unroll
    for (int i = 0; i < MT; ++i) {
        const int m = m_base + 32 * i + (lane & 31);
        e0[i] = (m < a.M && a.s0) ? a.s0[m] : 1.f;
        e1[i] = (MODE == MODE_FWD && m < a.M && a.s1) ? a.s1[m] : 0.f;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const bool relu = a.relu != 0;

    // ---- per-lane constants of the DMA: element offsets relative to (tile origin, chunk)
    long long xoff[XB];                              // src: row * cs + position
    int xrow[XB];
    unsigned xdst[XB];                               // LDS byte offset of the block inside a stage
#pragma unroll
    for (int j = 0; j < XB; ++j) {
        const int blk = wave * XB + j;               // 1 KB block of the stage
        const int kq = blk / NW, sb = blk - kq * NW; // row quad, group of four segments
        const int row = 4 * kq + ((lane >> 2) & 3), pos = 32 * (4 * sb + (lane >> 4)) + 8 * (lane & 3);
        xrow[j] = row;
        xoff[j] = (long long)row * a.src_cs + pos;
        xdst[j] = (unsigned)(kq * XQ + sb * 1024);
    }
    long long woff[WB];
    bool wok[WB];
    unsigned wdst[WB];
#pragma unroll
    for (int j = 0; j < WB; ++j) {
        const int blk = wave * WB + j, row = 16 * blk + (lane >> 2);
        const int q = (lane & 3) ^ ((row >> 2) & 3);
        wok[j] = m_base + row < a.Mpad;
        woff[j] = (long long)(m_base + row) * a.Kp + 8 * q;
        wdst[j] = (unsigned)(XS + blk * 1024);
    }
    // ---- fragment addresses (stage-relative)
    unsigned xfrag[2][NW][2];                        // [k16 step][position tile][half of the eight k]
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int j = 0; j < NW; ++j)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int kq = 4 * s + 2 * (lane >> 5) + h, rowin = (lane & 15) >> 2;
                const int seg = NW * wave + j;
                xfrag[s][j][h] = (unsigned)(kq * XQ + seg * 256 + rowin * 64 + (16 * ((lane >> 4) & 1) + 4 * (lane & 3)) * 2);
            }
    unsigned wfrag[2];                               // [k16 step]: row tile 0; + i * 2048 for row tile i
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int row = lane & 31, q = 2 * s + (lane >> 5);
        wfrag[s] = (unsigned)(XS + row * 64 + ((q ^ ((row >> 2) & 3)) * 16));
    }

    lds_byte* const lds0 = (lds_byte*)smem;
    const unsigned smem_lds = (unsigned)(size_t)lds0;            // LDS byte address of the ring
    unsigned char* const patch = smem + RING * STAGE + wave * (32 * EP);

    // ---- cursors: (tile of my list, chunk) of the item being LOADED and of the item being MULTIPLIED
    int l_tile = slot, l_chunk = 0;
    auto tile_origin = [&](int t, long long bs, int& b, int& p0) __attribute__((always_inline)) {
        b = t / a.tps;
        p0 = (t - b * a.tps) * BN;
        return (long long)b * bs + p0;
    };
    long long l_org;                                 // element offset of the load tile's first position in src
    {
        int b, p0;
        l_org = tile_origin(l_tile, a.src_bs, b, p0);
    }
    auto issue = [&](int stage) __attribute__((always_inline)) {
        const int k0 = l_chunk * KC;
        const long long xo = l_org + (long long)k0 * a.src_cs;
        const unsigned st = __builtin_amdgcn_readfirstlane(smem_lds + stage * STAGE);
#pragma unroll
        for (int j = 0; j < XB; ++j) {
            const void* g = k0 + xrow[j] < a.K ? (const void*)(a.src + xo + xoff[j]) : (const void*)a.zero;
            dma16(g, st + xdst[j]);
        }
#pragma unroll
        for (int j = 0; j < WB; ++j) {
            const void* g = wok[j] ? (const void*)(a.wp + woff[j] + k0) : (const void*)a.zero;
            dma16(g, st + wdst[j]);
        }
        if (++l_chunk == NC) {
            l_chunk = 0;
            l_tile += a.wgs;
            int b, p0;
            l_org = tile_origin(l_tile < a.tiles ? l_tile : slot, a.src_bs, b, p0);      // (past the end: a harmless re-read)
        }
    };

    f32x16 acc[MT][NW];
    auto clear = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int j = 0; j < NW; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    };
    auto multiply = [&](int stage) __attribute__((always_inline)) {
        lds_byte* const st = lds0 + stage * STAGE;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            bf16x8 xv[NW], wv[MT];
#pragma unroll
            for (int j = 0; j < NW; ++j) {
                const v4s16 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4s16*)(st + xfrag[s][j][0]));
                const v4s16 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4s16*)(st + xfrag[s][j][1]));
                xv[j] = bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
            }
#pragma unroll
            for (int i = 0; i < MT; ++i)
                wv[i] = *reinterpret_cast<const bf16x8*>(smem + stage * STAGE + wfrag[s] + i * 2048);
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int j = 0; j < NW; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xv[j], wv[i], acc[i][j], 0, 0, 0);
        }
    };
    // finished tile -> bf16 -> this wave's LDS patch -> 16-byte pieces.  acc[i][j][r]: position (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
    // of position tile j, channel 32 i + (lane & 31).
    auto finish = [&](int t) __attribute__((always_inline)) {
        int b, p0;
        const unsigned o_tile = (unsigned)(tile_origin(t, a.out_bs, b, p0) * 2);
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            if (m_base + 32 * i >= a.M) continue;                       // (uniform) a row tile past the layer's channels
            constexpr int NP = 2 * NW;                                   // pieces per lane: 32 rows x 4 NW pieces / 64 lanes
            unsigned ovo[NP];
            Words4 mk[NP];
#pragma unroll
            for (int u = 0; u < NP; ++u) {
                const int id = lane + 64 * u, row = id / (4 * NW), q = id - row * (4 * NW);
                const int m = m_base + 32 * i + row;
                ovo[u] = m < a.M ? (unsigned)(((long long)m * a.out_cs + 32 * NW * wave + 8 * q) * 2) : OOB;
                if constexpr (MODE == MODE_DGRAD)
                    if (a.mask) mk[u] = __builtin_bit_cast(Words4, __builtin_amdgcn_raw_buffer_load_b128(rm, ovo[u], o_tile, 0));
            }
#pragma unroll
            for (int j = 0; j < NW; ++j)
#pragma unroll
                for (int q4 = 0; q4 < 4; ++q4) {
                    float v[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        float x = acc[i][j][4 * q4 + e];
                        if constexpr (MODE == MODE_FWD) {
                            x = x * e0[i] + e1[i];
                            if (relu) x = fmaxf(x, 0.f);
                        } else {
                            x *= e0[i];
                        }
                        v[e] = x;
                    }
                    Words2 pk;
                    pk.a = cvt_pk_bf16(v[0], v[1]);
                    pk.b = cvt_pk_bf16(v[2], v[3]);
                    *reinterpret_cast<Words2A*>(patch + (lane & 31) * EP + (32 * j + 8 * q4 + 4 * (lane >> 5)) * 2) = pk;
                }
            // the patch is written and read by DIFFERENT lanes of this wave through differently typed accesses: the types
            // carry may_alias and the scheduler may not move LDS traffic across this point
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < NP; ++u) {
                const int id = lane + 64 * u, row = id / (4 * NW), q = id - row * (4 * NW);
                Words4 v = *reinterpret_cast<const Words4A*>(patch + row * EP + q * 16);
                if constexpr (MODE == MODE_DGRAD)
                    if (a.mask) {
                        v.a &= bf16_relu_mask2(mk[u].a); v.b &= bf16_relu_mask2(mk[u].b);
                        v.c &= bf16_relu_mask2(mk[u].c); v.d &= bf16_relu_mask2(mk[u].d);
                    }
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), ro, ovo[u], o_tile, 0);
            }
            // gfx9 hazard: a VALU write to the data registers of a 128-bit VMEM store with an SGPR offset needs one wait state
            // behind the store.  hipcc 7.2 counts the (instruction-less) wave barrier below as that wait state and lets the
            // accumulator clear (v_mov v15, 0) follow the store directly: the last dword of the last piece then left as 0.0
            // for the lanes whose data was fetched last (found in the ISA; 0.04 % of the outputs of one shape).
            asm volatile("s_nop 1" ::: "memory");
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();                            // the patch is free for the next row tile
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            __builtin_amdgcn_sched_barrier(0);
        }
    };

    // ---- the pipeline over the flattened (tile, chunk) sequence: a ring of three LDS stages, the DMA two items ahead.
    // Iteration `it`: DMA of item it+2 -> multiply item it -> wait until only the newest item's DMA is outstanding (item it+1
    // has landed; the count is by hand, in issue order: [stores of an earlier epilogue][item it+1][item it+2]) -> barrier ->
    // the tile's epilogue if this was its last chunk (after the barrier: the other waves go on with item it+1 meanwhile).
    issue(0);
    if (items > 1) issue(1);
    if (items > 1) dma_wait<L>(); else dma_wait<0>();
    __builtin_amdgcn_s_barrier();
    clear();
    int c_tile = slot, c_chunk = 0, stage = 0;
    for (int it = 0; it < items; ++it) {
        int nxt = stage + 2; if (nxt >= RING) nxt -= RING;
        if (it + 2 < items) issue(nxt);
        __builtin_amdgcn_sched_barrier(0);
        multiply(stage);
        __builtin_amdgcn_sched_barrier(0);
        if (it + 2 < items) dma_wait<L>(); else dma_wait<0>();
        __builtin_amdgcn_s_barrier();
        if (++c_chunk == NC) {
            finish(c_tile);
            clear();
            c_chunk = 0;
            c_tile += a.wgs;
        }
        if (++stage == RING) stage = 0;
    }
}

// the launch: tile shape, grid (eligibility: conv_select.h)
template <int MODE>
static int launch_conv1x1_stream(const ConvArgs& a, const unsigned short* wp, size_t wp_bytes, int Mpad, hipStream_t st) {
    const ConvGeom& g = a.g;
    S1Args s = {};
    const int P = (int)conv_out_positions(g);
    s.src = reinterpret_cast<const unsigned short*>(MODE == MODE_FWD ? a.x : a.dy);
    s.wp = wp;
    s.out = reinterpret_cast<unsigned short*>(a.out);
    s.mask = MODE == MODE_DGRAD ? reinterpret_cast<const unsigned short*>(a.emask) : nullptr;
    s.s0 = MODE == MODE_FWD ? a.scale : a.escale;
    s.s1 = MODE == MODE_FWD ? a.shift : nullptr;
    s.src_bs = MODE == MODE_FWD ? g.x_bs : g.y_bs; s.src_cs = MODE == MODE_FWD ? g.x_cs : g.y_cs;
    s.out_bs = MODE == MODE_FWD ? g.y_bs : g.x_bs; s.out_cs = MODE == MODE_FWD ? g.y_cs : g.x_cs;
    const int Cs = MODE == MODE_FWD ? g.Cin : g.Cout;
    (void)Cs; (void)wp_bytes;
    // 16-byte pieces on both sides: the DMA and the epilogue move eight bf16 positions per lane (the callers have checked
    // this for the layouts they route here; a foreign caller gets an error, not a misaligned access)
    if (((uintptr_t)s.src | (uintptr_t)s.out | (uintptr_t)s.wp) & 15) return OTAL_E_UNSUPPORTED;
    if ((s.src_bs | s.src_cs | s.out_bs | s.out_cs) & 7) return OTAL_E_UNSUPPORTED;
    if (s.mask && ((uintptr_t)s.mask & 15)) return OTAL_E_UNSUPPORTED;
    const int64_t ob = 2 * ((int64_t)(g.B - 1) * s.out_bs + (int64_t)(a.M - 1) * s.out_cs + P);
    if (ob >= (int64_t)0x7ffffff0) return OTAL_E_UNSUPPORTED;
    s.out_bytes = (unsigned)ob;
    s.zero = zero_word_address();
    if (!s.zero) return OTAL_E_UNSUPPORTED;
    s.M = a.M; s.Mpad = Mpad; s.K = a.K; s.Kp = chunk_kp(a.K); s.P = P;
    s.relu = (a.flags & EPI_RELU) ? 1 : 0;
    // tile shape: up to 6 row tiles per wave at 128 positions, up to 4 at 256 (only where the grid stays full)
    const int mt_all = (a.M + 31) / 32;
    int nw = 1;
    // (256-position tiles only with up to two row tiles per wave: the <4, 2> form needed 92 KB of LDS -- one workgroup per CU
    //  under a grid sized for two, DMA destinations past M0's 64 KB -- and no layer of the model selected it: removed)
    if (mt_all <= 2 && P % 256 == 0 && (int64_t)g.B * (P / 256) >= 1024) nw = 2;
    const int cap = nw == 2 ? 2 : 6;
    const int msplit = (mt_all + cap - 1) / cap;
    int mt = (mt_all + msplit - 1) / msplit;
    mt = (mt + 1) & ~1;                                       // instantiated: 2, 4, 6
    const int BN = 128 * nw;
    s.tps = P / BN;
    s.tiles = g.B * s.tps;
    int wgs = 512 / msplit;                                   // two workgroups per CU in all
    if (wgs > s.tiles) wgs = s.tiles;
    wgs = (wgs + 7) & ~7;                                     // sibling row groups of a tile on one XCD
    s.wgs = wgs;
    const dim3 grid((unsigned)(wgs * msplit));
#define OTAL_LAUNCH_S1(MT_, NW_) hipLaunchKernelGGL((conv1x1_stream_kernel<MT_, NW_, MODE>), grid, dim3(256), 0, st, s)
    if (nw == 2) OTAL_LAUNCH_S1(2, 2);
    else if (mt <= 2) OTAL_LAUNCH_S1(2, 1);
    else if (mt <= 4) OTAL_LAUNCH_S1(4, 1);
    else OTAL_LAUNCH_S1(6, 1);
#undef OTAL_LAUNCH_S1
    return otal_launch_status();
}
