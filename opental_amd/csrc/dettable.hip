// opental_amd/csrc/dettable.hip -- the Soft-NMS output of otal_softnms_classes_ws as one compact detection table on gfx950
// (the host loops it replaces: get_video_prediction, AFSD/anet/test.py:159-200; get_video_detections,
// AFSD/thumos14/test.py:165-200; the known-ness scores of threshold.py:128-147).  The rule is stated once in
// opental_amd/common/det_table.py (table_reference); this file is its device form, otal_detection_table.
//
// Three launches on the caller's stream, no allocation, no synchronisation, no atomic:
//   1. count   one workgroup of 256 threads per (video, class) list counts its valid rows into list_start[g + 1];
//   2. prefix  one workgroup turns the counts into the exclusive prefix list_start (V*K + 1), list_start[V*K] = N;
//   3. fill    the workgroups of pass 1 evaluate the same rows again and write them at list_start[g] + rank, rank = the
//              number of valid rows before row i in the list (a ballot per wave, the waves' counts through LDS).
// A row's position is therefore a function of the input alone: the table is (v, c, i) ascending and identical run to run.
// A list is read in chunks of 256 rows, each chunk as one contiguous run of 256 * cols floats through LDS (rows of 3 or 5
// floats would otherwise be read with a stride), and only up to counts[g]: rows past the count are never touched.
// Known-ness is fp64 from the fp32 columns, operation by operation as the Python lambdas of thumos14/test.py: OOD_SCORES;
// the library is built with -ffp-contract=off and nothing here calls fma.
#include "common.h"

#include <limits.h>

namespace {

constexpr int DT_THREADS = 256;
constexpr int DT_WAVES = DT_THREADS / OTAL_WAVE;
constexpr int DT_MAX_COLS = 5;

__device__ __forceinline__ double known_score(int scoring, double s, double u, double a) {
    switch (scoring) {
    case 0: return 1.0 - u;                                     // uncertainty
    case 1: { const double ood = 1.0 - s; return 1.0 - ood; }   // confidence
    case 2: { const double ood = u * a; return 1.0 - ood; }     // uncertainty_actionness
    case 3: { const double den = (1.0 - u) + 1e-6; const double ood = a / den; return 1.0 - ood; }   // a_by_inv_u
    case 4: { const double den = (1.0 - a) + 1e-6; const double ood = u / den; return 1.0 - ood; }   // u_by_inv_a
    default: { const double h = 0.5 * (a + 1.0); const double ood = h * u; return 1.0 - ood; }       // half_au
    }
}

// FILL false: list_start[g + 1] = the number of valid rows of list g.  FILL true: the rows are written.
template <bool FILL>
__global__ __launch_bounds__(DT_THREADS) void dettable_kernel(const float* __restrict__ rows, const int* __restrict__ counts,
                                                              const double* __restrict__ durations, int K, int top_k, int cols,
                                                              int clip, int scoring, int* __restrict__ video,
                                                              int* __restrict__ cls, double* __restrict__ seg,
                                                              float* __restrict__ sup, double* __restrict__ known,
                                                              int* __restrict__ list_start) {
    __shared__ float s_rows[DT_THREADS * DT_MAX_COLS];
    __shared__ int s_wave[DT_WAVES];
    const int g = blockIdx.x, tid = threadIdx.x, lane = tid & (OTAL_WAVE - 1), wave = tid / OTAL_WAVE;
    const int v = g / K;
    const int n = min(max(counts[g], 0), top_k);
    const float* list = rows + (size_t)g * top_k * cols;
    const double duration = durations ? durations[v] : 0.0;
    int running = FILL ? list_start[g] : 0;         // valid rows of this list before the current chunk (+ the list's start)
    for (int base = 0; base < n; base += DT_THREADS) {
        const int nrow = min(DT_THREADS, n - base);
        for (int e = tid; e < nrow * cols; e += DT_THREADS) s_rows[e] = list[(size_t)base * cols + e];
        __syncthreads();
        bool ok = false;
        double start = 0.0, end = 0.0;
        float sc = 0.0f, un = 0.0f, ac = 0.0f;
        if (tid < nrow) {
            const float* r = s_rows + tid * cols;
            sc = r[2];
            if (cols > 3) un = r[3];
            if (cols > 4) ac = r[4];
            start = (double)r[0];
            end = (double)r[1];
            ok = sc > 0.0f;                                     // false for NaN
            if (clip) {
                start = start > 0.0 ? start : 0.0;              // Python's max(0, start)
                if (durations) end = end < duration ? end : duration;   // Python's min(duration, end)
                if (end <= start) ok = false;
            }
        }
        const unsigned long long ballot = __ballot(ok);
        if (lane == 0) s_wave[wave] = __popcll(ballot);
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < DT_WAVES; ++w) {
            const int c = s_wave[w];
            if (w < wave) before += c;
            total += c;
        }
        if (FILL && ok) {
            const size_t p = (size_t)(running + before + __popcll(ballot & ((1ull << lane) - 1ull)));
            video[p] = v;
            cls[p] = g - v * K;
            seg[2 * p] = start;
            seg[2 * p + 1] = end;
            sup[3 * p] = sc;
            sup[3 * p + 1] = un;
            sup[3 * p + 2] = ac;
            known[p] = known_score(scoring, (double)sc, (double)un, (double)ac);
        }
        running += total;
        __syncthreads();            // s_rows and s_wave are rewritten by the next chunk
    }
    if (!FILL && tid == 0) list_start[g + 1] = running;
}

// list_start[0] = 0 and list_start[1 .. G] (the lists' counts) become their inclusive sums, in place: chunks of 256 with a
// carry, a Hillis-Steele scan inside a chunk.
__global__ __launch_bounds__(DT_THREADS) void dettable_prefix_kernel(int* __restrict__ list_start, int G) {
    __shared__ int s_scan[DT_THREADS];
    const int tid = threadIdx.x;
    int carry = 0;
    if (tid == 0) list_start[0] = 0;
    for (int base = 0; base < G; base += DT_THREADS) {
        const int j = base + tid;
        int x = j < G ? list_start[1 + j] : 0;
        s_scan[tid] = x;
        __syncthreads();
        for (int off = 1; off < DT_THREADS; off <<= 1) {
            const int y = tid >= off ? s_scan[tid - off] : 0;
            __syncthreads();
            x += y;
            s_scan[tid] = x;
            __syncthreads();
        }
        if (j < G) list_start[1 + j] = carry + x;
        carry += s_scan[DT_THREADS - 1];
        __syncthreads();            // s_scan is rewritten by the next chunk
    }
}

}  // namespace

extern "C" int otal_detection_table(const float* rows, const int* counts, const double* durations, int V, int K, int top_k,
                                    int cols, int drop_empty, int scoring, int* video, int* cls, double* seg, float* sup,
                                    double* known, int* list_start, void* stream) {
    if (!rows || !counts || !video || !cls || !seg || !sup || !known || !list_start) return OTAL_E_NULL;
    if (V <= 0 || K <= 0 || top_k <= 0 || cols < 3 || cols > DT_MAX_COLS) return OTAL_E_SHAPE;
    if (scoring < 0 || scoring > 5) return OTAL_E_UNSUPPORTED;
    if ((long long)V * K * top_k > (long long)INT_MAX) return OTAL_E_UNSUPPORTED;    // positions are int32
    const int G = V * K, clip = (durations != nullptr || drop_empty != 0) ? 1 : 0;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(dettable_kernel<false>, dim3(G), dim3(DT_THREADS), 0, st, rows, counts, durations, K, top_k, cols, clip,
                       scoring, video, cls, seg, sup, known, list_start);
    hipLaunchKernelGGL(dettable_prefix_kernel, dim3(1), dim3(DT_THREADS), 0, st, list_start, G);
    hipLaunchKernelGGL(dettable_kernel<true>, dim3(G), dim3(DT_THREADS), 0, st, rows, counts, durations, K, top_k, cols, clip,
                       scoring, video, cls, seg, sup, known, list_start);
    return otal_launch_status();
}
