// opental_amd/csrc/rplhead.hip -- the distance head of the RPL / GCPL baselines (reference AFSD/common/layers.py:314-351,
// RPLHead with one centre per class and the 'l2' metric), forward and backward, on the channel-major maps of the pyramid.
//
//   dist[b][c][n]   = 1/D * sum_d (x[b][d][n] - centers[c][d])^2
//   dx[b][d][n]     = 2/D * sum_c g[b][c][n] * (x[b][d][n] - centers[c][d])
//   dcenters[c][d]  = 2/D * sum_{b,n} g[b][c][n] * (centers[c][d] - x[b][d][n])
//
// The reference permutes the map to (B N, D), evaluates |f|^2 - 2 f.c + |c|^2 with a matmul and permutes the result back
// (six ATen launches forward, a dozen backward).  Here the map is read where it lies, the distance is the direct sum of
// squared differences in fp32 (no cancellation between the three expanded terms) and every sum runs in one fixed order:
// plain stores, no floating-point atomics, two runs give the same bits.
//
// The op is small (B 8, N 126, C 16, D 512: 16 MFLOP) and bound by launch and latency, so the tiling aims at ONE launch
// with coalesced reads along N and the centres staged once per workgroup in LDS (16 x 512 floats = 32 KB), not at occupancy:
//   forward / dx   grid (ceil(N / 32), B), 256 threads = 32 columns x 8 channel groups.  A thread walks the channels
//                  4 * (g + 8 j) .. + 3 of its group g (one 16-byte LDS read per centre, the same address for the 32 lanes
//                  of a group: a broadcast) and keeps one accumulator per class; the eight partial sums of a (class, column)
//                  are added in group order through LDS, which the centres no longer need by then.
//   dcenters       grid D / 16, 256 threads = 4 waves x 4 channels each; the lanes run along N (coalesced reads of x and g),
//                  batch by batch, and a fixed shuffle tree adds the 64 lane sums of every (class, channel).
#include "common.h"

namespace {

constexpr int RH_MAX_C = 21;        // classes (centres): the accumulators of a thread
constexpr int RH_MAX_D = 512;       // feature channels: the LDS-resident centre table
constexpr int RH_TN = 32;           // columns of a forward / dx workgroup
constexpr int RH_DG = 8;            // channel groups of a forward / dx workgroup
constexpr int RH_THREADS = RH_TN * RH_DG;
constexpr int RH_WD = 4;            // channels per wave of the dcenters kernel
constexpr int RH_WAVES = 4;

struct RplArgs {
    const float* x;         // (B, D, N)
    const float* centers;   // (C, D)
    const float* g;         // (B, C, N)    backward
    float* dist;            // (B, C, N)    forward
    float* dx;              // (B, D, N)
    float* dcenters;        // (C, D)
    int B, C, D, N;
};

__device__ __forceinline__ void stage_centers(float* cl, const float* centers, int CD) {
    // (C, D) row-major, D % 16 == 0: 16-byte pieces when the table allows, element-wise otherwise
    const int t = threadIdx.x;
    const int n4 = (reinterpret_cast<uintptr_t>(centers) & 15) == 0 ? CD >> 2 : 0;
    for (int q = t; q < n4; q += RH_THREADS) reinterpret_cast<float4*>(cl)[q] = reinterpret_cast<const float4*>(centers)[q];
    for (int q = 4 * n4 + t; q < CD; q += RH_THREADS) cl[q] = centers[q];
}

__global__ __launch_bounds__(RH_THREADS) void rpl_head_fwd_kernel(const RplArgs a) {
    extern __shared__ __attribute__((aligned(16))) float cl[];      // centres (C * D), then the partial sums (RH_DG * C * RH_TN)
    const int t = threadIdx.x, nl = t & (RH_TN - 1), dg = t / RH_TN;
    const int b = blockIdx.y, n = blockIdx.x * RH_TN + nl;
    const int C = a.C, D = a.D, N = a.N;
    const bool live = n < N;
    stage_centers(cl, a.centers, C * D);
    __syncthreads();
    float acc[RH_MAX_C];
#pragma unroll
    for (int c = 0; c < RH_MAX_C; ++c) acc[c] = 0.f;
    const float* xb = a.x + (size_t)b * D * N;
    for (int d4 = dg; d4 < (D >> 2); d4 += RH_DG) {
        const int d = d4 << 2;
        float f[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) f[u] = live ? xb[(size_t)(d + u) * N + n] : 0.f;
#pragma unroll
        for (int c = 0; c < RH_MAX_C; ++c)
            if (c < C) {
                const float4 cv = *reinterpret_cast<const float4*>(cl + c * D + d);
                const float e0 = f[0] - cv.x, e1 = f[1] - cv.y, e2 = f[2] - cv.z, e3 = f[3] - cv.w;
                acc[c] += e0 * e0;
                acc[c] += e1 * e1;
                acc[c] += e2 * e2;
                acc[c] += e3 * e3;
            }
    }
    __syncthreads();            // every read of the centres is done: the region now holds the partial sums
#pragma unroll
    for (int c = 0; c < RH_MAX_C; ++c)
        if (c < C) cl[(dg * C + c) * RH_TN + nl] = acc[c];
    __syncthreads();
    for (int e = t; e < C * RH_TN; e += RH_THREADS) {
        const int c = e / RH_TN, col = e - c * RH_TN;
        const int nn = blockIdx.x * RH_TN + col;
        float s = 0.f;
#pragma unroll
        for (int gI = 0; gI < RH_DG; ++gI) s += cl[(gI * C + c) * RH_TN + col];     // group order
        if (nn < N) a.dist[((size_t)b * C + c) * N + nn] = s / (float)D;
    }
}

__global__ __launch_bounds__(RH_THREADS) void rpl_head_dx_kernel(const RplArgs a) {
    extern __shared__ __attribute__((aligned(16))) float cl[];      // centres (C * D)
    const int t = threadIdx.x, nl = t & (RH_TN - 1), dg = t / RH_TN;
    const int b = blockIdx.y, n = blockIdx.x * RH_TN + nl;
    const int C = a.C, D = a.D, N = a.N;
    const bool live = n < N;
    stage_centers(cl, a.centers, C * D);
    float gv[RH_MAX_C];
#pragma unroll
    for (int c = 0; c < RH_MAX_C; ++c) gv[c] = (c < C && live) ? a.g[((size_t)b * C + c) * N + n] : 0.f;
    __syncthreads();
    const float* xb = a.x + (size_t)b * D * N;
    float* dxb = a.dx + (size_t)b * D * N;
    const float k = 2.f / (float)D;
    for (int d4 = dg; d4 < (D >> 2); d4 += RH_DG) {
        const int d = d4 << 2;
        float f[4], s[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int u = 0; u < 4; ++u) f[u] = live ? xb[(size_t)(d + u) * N + n] : 0.f;
#pragma unroll
        for (int c = 0; c < RH_MAX_C; ++c)
            if (c < C) {                                                            // class order
                const float4 cv = *reinterpret_cast<const float4*>(cl + c * D + d);
                s[0] += gv[c] * (f[0] - cv.x);
                s[1] += gv[c] * (f[1] - cv.y);
                s[2] += gv[c] * (f[2] - cv.z);
                s[3] += gv[c] * (f[3] - cv.w);
            }
        if (live) {
#pragma unroll
            for (int u = 0; u < 4; ++u) dxb[(size_t)(d + u) * N + n] = k * s[u];
        }
    }
}

__global__ __launch_bounds__(RH_WAVES * 64) void rpl_head_dcenters_kernel(const RplArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int d0 = (blockIdx.x * RH_WAVES + wave) * RH_WD;      // D % 16 == 0: every wave owns four channels
    const int C = a.C, D = a.D, N = a.N;
    float cen[RH_WD][RH_MAX_C], acc[RH_WD][RH_MAX_C];
#pragma unroll
    for (int u = 0; u < RH_WD; ++u)
#pragma unroll
        for (int c = 0; c < RH_MAX_C; ++c) {
            cen[u][c] = c < C ? a.centers[(size_t)c * D + d0 + u] : 0.f;
            acc[u][c] = 0.f;
        }
    for (int b = 0; b < a.B; ++b) {                              // batch order, then column order
        const float* xb = a.x + ((size_t)b * D + d0) * N;
        const float* gb = a.g + (size_t)b * C * N;
        for (int n = lane; n < N; n += 64) {
            float f[RH_WD];
#pragma unroll
            for (int u = 0; u < RH_WD; ++u) f[u] = xb[(size_t)u * N + n];
#pragma unroll
            for (int c = 0; c < RH_MAX_C; ++c)
                if (c < C) {
                    const float gv = gb[(size_t)c * N + n];
#pragma unroll
                    for (int u = 0; u < RH_WD; ++u) acc[u][c] += gv * (cen[u][c] - f[u]);
                }
        }
    }
    const float k = 2.f / (float)D;
#pragma unroll
    for (int u = 0; u < RH_WD; ++u)
#pragma unroll
        for (int c = 0; c < RH_MAX_C; ++c)
            if (c < C) {
                float r = acc[u][c];
#pragma unroll
                for (int s = 32; s > 0; s >>= 1) r += __shfl_down(r, s, 64);       // the halving tree over the lanes
                if (lane == 0) a.dcenters[(size_t)c * D + d0 + u] = k * r;
            }
}

int check(const void* x, const void* centers, int B, int C, int D, int N) {
    if (!x || !centers) return OTAL_E_NULL;
    if (B <= 0 || C <= 0 || D <= 0 || N <= 0) return OTAL_E_SHAPE;
    if (C > RH_MAX_C || D > RH_MAX_D || D % 16 || B > 65535) return OTAL_E_UNSUPPORTED;
    return 0;
}

}  // namespace

extern "C" int otal_rpl_head_fwd(const float* x, const float* centers, float* dist, int B, int C, int D, int N, void* stream) {
    if (!dist) return OTAL_E_NULL;
    if (int e = check(x, centers, B, C, D, N)) return e;
    RplArgs a{};
    a.x = x; a.centers = centers; a.dist = dist; a.B = B; a.C = C; a.D = D; a.N = N;
    const size_t fl = (size_t)C * D > (size_t)RH_DG * C * RH_TN ? (size_t)C * D : (size_t)RH_DG * C * RH_TN;
    hipLaunchKernelGGL(rpl_head_fwd_kernel, dim3((N + RH_TN - 1) / RH_TN, B), dim3(RH_THREADS), fl * sizeof(float),
                       (hipStream_t)stream, a);
    return otal_launch_status();
}

extern "C" int otal_rpl_head_bwd(const float* x, const float* centers, const float* g, float* dx, float* dcenters, int B, int C,
                                 int D, int N, int parts, void* stream) {
    if (!g) return OTAL_E_NULL;
    if (int e = check(x, centers, B, C, D, N)) return e;
    if (parts < 1 || parts > 3) return OTAL_E_SHAPE;
    if ((parts & 2) && !dcenters) return OTAL_E_NULL;
    RplArgs a{};
    a.x = x; a.centers = centers; a.g = g; a.dx = dx; a.dcenters = dcenters; a.B = B; a.C = C; a.D = D; a.N = N;
    if ((parts & 1) && dx) {
        hipLaunchKernelGGL(rpl_head_dx_kernel, dim3((N + RH_TN - 1) / RH_TN, B), dim3(RH_THREADS), (size_t)C * D * sizeof(float),
                           (hipStream_t)stream, a);
        if (int e = otal_launch_status()) return e;
    }
    if (!(parts & 2)) return 0;
    hipLaunchKernelGGL(rpl_head_dcenters_kernel, dim3(D / (RH_WAVES * RH_WD)), dim3(RH_WAVES * 64), 0, (hipStream_t)stream, a);
    return otal_launch_status();
}
