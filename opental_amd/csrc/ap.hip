// opental_amd/csrc/ap.hip -- average precision per (class, tIoU threshold) from the codes of otal_eval_match on gfx950
// (AFSD/evaluation/eval_detection.py: the tail of compute_average_precision_detection :388-402 and
// utils_eval.interpolated_prec_rec :20-29, which run per class on the host).  The rule is stated once in
// opental_amd/evaluation/table_ap.py (ap_reference); this file is its device form, otal_average_precision.
//
// One workgroup of AP_TILE = 256 threads owns one (class, threshold) pair; pairs are independent, so nothing crosses a
// workgroup: no atomic, no scratch, no flag.  The class's rows r = 0 .. n-1 (descending score) are walked in chunks of AP_TILE,
// one row per thread, twice:
//   1. count    the class's true positives (tp_r = codes[t][rank_pos[r]] >= 0), int32, no barrier inside the loop;
//   2. back     the chunks from the LAST to the first.  A chunk's tp count gives the cumulative count at its start (the count
//               at its end is carried: the class total for the last chunk), a ballot prefix gives tp_cum_r;
//               precision_r = tp_cum_r / (r + 1); the envelope max over j >= r is a suffix maximum inside the wave (shuffles),
//               across the chunk's waves (LDS) and the carried maximum of the chunks behind; the rows with tp_r = 1 contribute
//               (tp_cum_r / npos - (tp_cum_r - 1) / npos) * envelope_r.
// The contributions of a chunk are summed by a butterfly inside each wave, the four waves' sums in wave order, and the chunks'
// sums from the last chunk to the first: an order fixed by AP_TILE and the class size alone, whatever the grid.  All of it is
// fp64 with IEEE division (the library is built with -ffp-contract=off and nothing here calls fma).
// Every barrier sits in a loop whose trip count comes from class_start alone, so all threads reach it.  class_start is
// clamped into 0 .. N and a position outside 0 .. N-1 counts as a false positive: no input makes the kernel read out of bounds.
#include "common.h"

#include <limits.h>

namespace {

constexpr int AP_TILE = OTAL_AP_TILE;
constexpr int AP_WAVES = AP_TILE / OTAL_WAVE;
static_assert(AP_TILE % OTAL_WAVE == 0 && AP_WAVES == 4, "the wave sums are added as ((s0 + s1) + s2) + s3");

__global__ __launch_bounds__(AP_TILE) void average_precision_kernel(const int* __restrict__ codes,
                                                                    const int* __restrict__ rank_pos,
                                                                    const int* __restrict__ class_start,
                                                                    const int* __restrict__ gt_count, int N, int K,
                                                                    double* __restrict__ ap) {
    __shared__ int s_cnt[AP_WAVES];
    __shared__ double s_max[AP_WAVES];
    __shared__ double s_sum[AP_WAVES];
    const int c = blockIdx.x, t = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & (OTAL_WAVE - 1), wave = tid / OTAL_WAVE;
    const int c0 = clampi(class_start[c], 0, N), c1 = clampi(class_start[c + 1], c0, N);
    const int n = c1 - c0;
    const int nchunks = (n + AP_TILE - 1) / AP_TILE;
    if (nchunks == 0) {
        if (tid == 0) ap[(size_t)t * K + c] = 0.0;
        return;
    }
    const int* row = codes + (size_t)t * N;
    const double npos = (double)gt_count[c];

    // pass 1: the class's true positives
    int mine = 0;
    for (int r = c0 + tid; r < c1; r += AP_TILE) {
        const int pos = rank_pos[r];
        mine += ((unsigned)pos < (unsigned)N && row[pos] >= 0) ? 1 : 0;
    }
    for (int off = OTAL_WAVE / 2; off > 0; off >>= 1) mine += __shfl_xor(mine, off, OTAL_WAVE);
    if (lane == 0) s_cnt[wave] = mine;
    __syncthreads();
    int end_cum = 0;                    // true positives up to the end of the current chunk
    for (int w = 0; w < AP_WAVES; ++w) end_cum += s_cnt[w];
    __syncthreads();                    // s_cnt is rewritten by the first chunk

    // pass 2: the chunks from the back
    double carry_max = 0.0;             // the envelope of the rows behind the current chunk (the appended precision 0)
    double acc = 0.0;
    for (int k = nchunks - 1; k >= 0; --k) {
        const int rr = k * AP_TILE + tid;           // rank inside the class
        const bool valid = rr < n;
        bool tp = false;
        if (valid) {
            const int pos = rank_pos[c0 + rr];
            tp = (unsigned)pos < (unsigned)N && row[pos] >= 0;
        }
        const unsigned long long ballot = __ballot(tp);
        if (lane == 0) s_cnt[wave] = __popcll(ballot);
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < AP_WAVES; ++w) {
            const int x = s_cnt[w];
            if (w < wave) before += x;
            total += x;
        }
        const int start_cum = end_cum - total;
        const int tp_cum = start_cum + before + __popcll(ballot & ((2ull << lane) - 1ull));      // inclusive of this row
        const double prec = valid ? (double)tp_cum / (double)(rr + 1) : 0.0;
        double suf = prec;                          // max over the lanes >= this one
        for (int off = 1; off < OTAL_WAVE; off <<= 1) {
            const double o = __shfl_down(suf, off, OTAL_WAVE);
            if (lane + off < OTAL_WAVE && o > suf) suf = o;
        }
        if (lane == 0) s_max[wave] = suf;
        __syncthreads();
        double env = carry_max, chunk_max = carry_max;
        for (int w = 0; w < AP_WAVES; ++w) {
            const double x = s_max[w];
            if (w > wave && x > env) env = x;
            if (x > chunk_max) chunk_max = x;
        }
        if (suf > env) env = suf;
        double term = 0.0;
        if (tp) term = ((double)tp_cum / npos - (double)(tp_cum - 1) / npos) * env;
        for (int off = OTAL_WAVE / 2; off > 0; off >>= 1) term += __shfl_xor(term, off, OTAL_WAVE);
        if (lane == 0) s_sum[wave] = term;
        __syncthreads();
        acc += ((s_sum[0] + s_sum[1]) + s_sum[2]) + s_sum[3];
        carry_max = chunk_max;
        end_cum = start_cum;
        // s_cnt, s_max and s_sum are rewritten by the next chunk only after its own barriers: the reads above are behind one
    }
    if (tid == 0) ap[(size_t)t * K + c] = acc;
}

}  // namespace

extern "C" int otal_average_precision(const int* codes, const int* rank_pos, const int* class_start, const int* gt_count,
                                      int N, int K, int nthr, double* ap, void* stream) {
    if (!codes || !rank_pos || !class_start || !gt_count || !ap) return OTAL_E_NULL;
    if (N < 0 || K < 1 || nthr < 1) return OTAL_E_SHAPE;
    // a class holds at most N rows: the bound on a class is checked through N, without reading class_start from the device
    if (nthr > 32 || N > OTAL_AP_MAX_CLASS_ROWS) return OTAL_E_UNSUPPORTED;
    hipLaunchKernelGGL(average_precision_kernel, dim3(K, nthr), dim3(AP_TILE), 0, (hipStream_t)stream, codes, rank_pos,
                       class_start, gt_count, N, K, ap);
    return otal_launch_status();
}
