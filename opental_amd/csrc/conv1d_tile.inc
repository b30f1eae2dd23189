// opental_amd/csrc/conv1d_tile.inc -- included by conv_gemm.hip inside its anonymous namespace.
//
// Forward / data gradient of the 1-D temporal layers (Unit1D k = 1 / 3, stride 1, SAME; AFSD/common/layers.py:178-214 as
// used by the towers, ProposalBranches and the frame-level deconv of AFSD/thumos14/BDNet.py:67-113,:156-203) on the
// level-packed (B,C,126) / frame-level (B,C,256) maps, bf16 operands.
//
// These GEMMs are tiny (M <= 1024, N = 126 per sample, K <= 2048 x 3): on the tiled kernels above they ran as 32 output
// tiles x up to 16 K splits -> 33 MB of fp32 slabs written and re-read by a second (reduce) launch, ~20 us of GPU time
// for ~1.6 GFLOP.  Here a workgroup owns 32 output channels x 64 positions of one sample and streams the WHOLE K through LDS in
// chunks of 128 channels, double buffered:
//   * no split-K, no slabs, no second launch: the epilogue (bias / scale, ReLU) stores the final values;
//   * A = the persistent bf16 weight pack of the chunked path (k = ((c/8) * kt + tap) * 8 + c % 8): a chunk of channels is
//     a contiguous run of every row, copied with 16-byte loads;
//   * B = the source rows of the chunk, transposed while staged to [position][channel] bf16 cells (16-byte loads along the
//     positions, at 8-byte aligned addresses on the 126-float rows), so that the fragment of tap dt at position n is the 16
//     contiguous bytes of cell n + dt - 1 -- a tap is a cell shift, level boundaries and the tensor ends are a per-lane
//     zero select.
// grid = (ceil(M / 32), B * ceil(T / 64)): 256 .. 512 workgroups on the model's maps, one launch.
template <int KT, int MODE>
__global__ __launch_bounds__(256) void conv1d_tile_kernel(const ConvArgs a) {
    constexpr int NTL = 64;                                 // positions per workgroup (two 32-wide MFMA tiles)
    constexpr int KC = 128;                                 // channels per K chunk
    constexpr int CELLS = NTL + 8;                          // positions n0 - 4 .. n0 + NTL + 3
    constexpr int CP = KC * 2 + 16;                         // cell pitch (bytes): conflict-free 16-byte fragment reads
    constexpr int AP = KT * KC * 2 + 16;                    // A row pitch
    constexpr int XB = CELLS * CP, AB = 32 * AP;
    constexpr int NS = KC * KT / 16;                        // k16 steps per chunk (even: the two wave pairs take alternate steps)
    constexpr int B_ITEMS = (CELLS / 4) * (KC / 2), B_ITERS = (B_ITEMS + 255) / 256;    // (position quad, channel pair)
    constexpr int A_PIECES = 32 * (KT * KC / 8), A_ITERS = A_PIECES / 256;              // 16-byte pieces
    static_assert(A_PIECES % 256 == 0 && NS % 2 == 0, "tiling");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];                // [2][XB] [2][AB]
    const ConvGeom& g = a.g;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int T = g.Ti;
    const int nblk = (T + NTL - 1) / NTL;
    // Which XCD fetches what: workgroups go to the eight XCDs round-robin by linear index, so with the plain (x = row block,
    // y = position block) grid every XCD held two row blocks of ALL position blocks -- its L2 fetched the whole source map, eight
    // times 2 MB for a launch whose algorithmic traffic is 7.3 MB (counter / algorithmic 2.72, VERDICT r4 weak 4).  Here an XCD
    // owns a (half of the row blocks) x (quarter of the position blocks) rectangle: half of the weight pack + a quarter of
    // the map per L2 (counter 19.8 -> ~12 MB).  A bijection whenever the grid divides (2, 4); the plain map otherwise.
    int bx = blockIdx.x, by = blockIdx.y;
    if ((gridDim.x & 1) == 0 && (gridDim.y & 3) == 0) {
        const int lin = blockIdx.x + gridDim.x * blockIdx.y, xcd = lin & 7, idx = lin >> 3;
        const int hx = gridDim.x >> 1, qy = gridDim.y >> 2;
        bx = (xcd & 1) * hx + idx % hx;
        by = (xcd >> 1) * qy + idx / hx;
    }
    const int m0 = bx * 32;
    const int b = by / nblk, n0 = (by - b * nblk) * NTL;
    const int C = MODE == MODE_FWD ? g.Cin : g.Cout;        // channels of the gathered tensor
    const bool second = blockIdx.z != 0;                    // pair launch: grid.z = 2, same geometry, the other tensors
    const float* src = MODE == MODE_FWD ? (second ? a.x2 : a.x) : (second ? a.dy2 : a.dy);
    const int64_t sbs = MODE == MODE_FWD ? g.x_bs : g.y_bs, scs = MODE == MODE_FWD ? g.x_cs : g.y_cs;
    const int64_t obs = MODE == MODE_FWD ? g.y_bs : g.x_bs, ocs = MODE == MODE_FWD ? g.y_cs : g.x_cs;
    const auto rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(src), 0, (int)a.src_bytes, 0x00020000);
    const auto rw = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned short*>(second ? a.wp2 : a.wp), 0, (int)a.wp_bytes, 0x00020000);
    const int nchunks = C / KC;

    // ---- per-thread staging items.  A quad is 4 consecutive positions of one channel: a 16-byte load at an address that is
    // only 8-byte aligned on the 126-float rows (legal on gfx950, ~10 % slower than aligned: tools/ubench/alignprobe.hip).
    // Positions outside [0, T) are never zeroed: their cells are only reached through taps the level mask rejects.
    unsigned bvo[B_ITERS];
    int blds[B_ITERS];
#pragma unroll
    for (int i = 0; i < B_ITERS; ++i) {
        const int item = tid + 256 * i;
        const int q = item % (CELLS / 4), cp = item / (CELLS / 4);
        bvo[i] = item < B_ITEMS ? (unsigned)(((int64_t)b * sbs + (int64_t)(2 * cp) * scs + (n0 - 4 + 4 * q)) * 4) : 0xffffffffu;
        blds[i] = (4 * q) * CP + cp * 4;
    }
    unsigned avo[A_ITERS];
    int alds[A_ITERS];
#pragma unroll
    for (int j = 0; j < A_ITERS; ++j) {
        const int p = tid + 256 * j;
        const int m = p / (KT * KC / 8), q = p - m * (KT * KC / 8);
        avo[j] = (unsigned)(((int64_t)(m0 + m) * a.Kp) * 2 + q * 16);
        alds[j] = m * AP + q * 16;
    }
    // ---- this lane's output position and the taps that stay inside its level.  Waves 0/1 and 2/3 own the same two
    // position tiles and take alternate k16 steps of every chunk; the pairs' partial sums meet in LDS at the end.
    const int ntile = wave & 1, khalf = wave >> 1;
    const int nl = ntile * 32 + (lane & 31);
    const int n = n0 + nl;
    unsigned okm = 0;                                       // bit t: tap t usable at this position
    {
        int lo, up;
        level_bounds(g, n < T ? n : T - 1, T, lo, up);
#pragma unroll
        for (int t = 0; t < KT; ++t) {
            const int d = MODE == MODE_FWD ? t - g.pt : g.pt - t;
            okm |= (unsigned)(n < T && n + d >= lo && n + d < up) << t;
        }
    }
    const int ncell = (nl + 4) * CP;
    const int h = lane >> 5;

    Words4 rb[B_ITERS][2];
    Words4 ra[A_ITERS];
    auto load = [&](int chunk) {
        const int so = (int)((int64_t)chunk * KC * scs * 4);
#pragma unroll
        for (int i = 0; i < B_ITERS; ++i)
#pragma unroll
            for (int e = 0; e < 2; ++e)
                rb[i][e] = __builtin_bit_cast(Words4, __builtin_amdgcn_raw_buffer_load_b128(rs, bvo[i], so + (e ? (int)(scs * 4) : 0), 0));
        const int ao = chunk * (KC * KT * 2);
#pragma unroll
        for (int j = 0; j < A_ITERS; ++j)
            ra[j] = __builtin_bit_cast(Words4, __builtin_amdgcn_raw_buffer_load_b128(rw, avo[j], ao, 0));
    };
    auto store = [&](int buf) {
        unsigned char* X = smem + buf * XB;
        unsigned char* A = smem + 2 * XB + buf * AB;
#pragma unroll
        for (int i = 0; i < B_ITERS; ++i) {
            if (B_ITEMS % 256 != 0 && tid + 256 * i >= B_ITEMS) continue;
            *reinterpret_cast<unsigned*>(X + blds[i]) = cvt_pk_bf16(__uint_as_float(rb[i][0].a), __uint_as_float(rb[i][1].a));
            *reinterpret_cast<unsigned*>(X + blds[i] + CP) = cvt_pk_bf16(__uint_as_float(rb[i][0].b), __uint_as_float(rb[i][1].b));
            *reinterpret_cast<unsigned*>(X + blds[i] + 2 * CP) = cvt_pk_bf16(__uint_as_float(rb[i][0].c), __uint_as_float(rb[i][1].c));
            *reinterpret_cast<unsigned*>(X + blds[i] + 3 * CP) = cvt_pk_bf16(__uint_as_float(rb[i][0].d), __uint_as_float(rb[i][1].d));
        }
#pragma unroll
        for (int j = 0; j < A_ITERS; ++j) *reinterpret_cast<Words4*>(A + alds[j]) = ra[j];
    };

    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;

    load(0);
    store(0);
    __syncthreads();
    for (int c = 0; c < nchunks; ++c) {
        const int buf = c & 1;
        const bool more = c + 1 < nchunks;
        const unsigned char* X = smem + buf * XB;
        const unsigned char* A = smem + 2 * XB + buf * AB + (lane & 31) * AP + h * 16;
        if (more) load(c + 1);
#pragma unroll
        for (int s2 = 0; s2 < NS / 2; ++s2) {
            // this wave's step s = 2 s2 + khalf; its k8 groups: 2s (lanes 0..31) and 2s + 1 (lanes 32..63);
            // group q = (channel block q / KT, tap q % KT)
            const int q = 4 * s2 + 2 * khalf + h;
            const int cb = q / KT, tap = q - cb * KT;
            const int d = MODE == MODE_FWD ? tap - g.pt : g.pt - tap;
            const bf16x8 av = *reinterpret_cast<const bf16x8*>(A + (2 * s2 + khalf) * 32);
            bf16x8 bv = *reinterpret_cast<const bf16x8*>(X + ncell + d * CP + cb * 16);
            const bf16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
            bv = ((okm >> tap) & 1u) ? bv : zero;
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, bv, acc, 0, 0, 0);
        }
        if (more) store(buf ^ 1);
        __syncthreads();
    }
    // the epilogue's per-row operands: requested here (all 32 together, no value touched) so that they arrive under the hand-over
    // below -- fetched where they are used, `if (scale) x *= scale[m]` was a branch + full wait per row: 32 dependent loads
    const float* const scale = second ? a.scale2 : a.scale;
    const float* const shift = second ? a.shift2 : a.shift;
    float sc[16], sh[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) { sc[r] = 1.f; sh[r] = 0.f; }
    if constexpr (MODE == MODE_FWD) {
        if (scale) {
#pragma unroll
            for (int r = 0; r < 16; ++r) sc[r] = scale[min(m0 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5), a.M - 1)];
        }
        if (shift) {
#pragma unroll
            for (int r = 0; r < 16; ++r) sh[r] = shift[min(m0 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5), a.M - 1)];
        }
    }
    // ---- the odd-step waves hand their partial sums to the even-step ones (fixed order: even steps + odd steps)
    float* xch = reinterpret_cast<float*>(smem);            // 2 tiles x 16 x 64 floats = 8 KB (the operand buffers are free)
    if (khalf == 1) {
#pragma unroll
        for (int r = 0; r < 16; ++r) xch[(ntile * 16 + r) * 64 + lane] = acc[r];
    }
    __syncthreads();
    if (khalf == 1) return;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] += xch[(ntile * 16 + r) * 64 + lane];

    // ---- epilogue: final values (no split-K): FWD y = act(scale * acc + shift); DGRAD dx (+)= acc
    const auto ro = __builtin_amdgcn_make_buffer_rsrc(second ? a.out2 : a.out, 0, (int)a.out_bytes, 0x00020000);
    const bool relu = (a.flags & EPI_RELU) != 0, accum = (a.flags & EPI_ACCUM) != 0;
    unsigned vo[16];
    float v[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int m = m0 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        const bool ok = n < T && m < a.M;
        vo[r] = ok ? (unsigned)(((int64_t)b * obs + (int64_t)m * ocs + n) * 4) : 0xffffffffu;
        float x = acc[r];
        if constexpr (MODE == MODE_FWD) {
            if (scale) x *= sc[r];
            if (shift) x += sh[r];
            if (relu) x = fmaxf(x, 0.f);
        }
        v[r] = x;
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

template <int KT, int MODE>
static int launch_c1t(const ConvArgs& a, dim3 grid, hipStream_t st) {
    constexpr int lds = 2 * ((64 + 8) * (128 * 2 + 16) + 32 * (KT * 128 * 2 + 16));
    return launch_big_lds<conv1d_tile_kernel<KT, MODE>>(lds, grid, 256, st, a);
}

template <int MODE>
int launch_conv1d_tile(ConvArgs& a, const ConvLaunchShape& sh, void* ws, hipStream_t st) {
    // tables + packed weights: the persistent region of the chunked path (same layout), or built here in the workspace
    const int BMsel = choose_bm(a.M, true);
    a.Kp = chunk_kp(a.K);
    const size_t wb = chunk_wp_bytes(a.M, BMsel, a.K);
    int2* ctab;
    if (int e = chunk_region<MODE>(a, a.pre, ws, ctab, a.wp, st)) return e;
    if (a.pair) {           // the second problem's packed weights: its own persistent region, or built behind the first
        ConvArgs b = a;
        b.w = a.w2;
        if (int e = chunk_region<MODE>(b, a.pre2, static_cast<char*>(ws) + sh.second_at, ctab, a.wp2, st)) return e;
    }
    a.wp_bytes = (unsigned)wb;
    a.src_bytes = (unsigned)gather_extent_bytes(a.g, MODE);
    if (!set_splits<MODE>(a, sh, ws)) return OTAL_E_UNSUPPORTED;
    const dim3 grid(sh.grid[0], sh.grid[1], sh.grid[2]);
    return a.g.kt == 3 ? launch_c1t<3, MODE>(a, grid, st) : launch_c1t<1, MODE>(a, grid, st);
}
