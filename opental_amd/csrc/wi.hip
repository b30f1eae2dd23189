// opental_amd/csrc/wi.hip -- Wilderness Impact per (class, tIoU threshold) from the codes of otal_eval_match_labeled on gfx950
// (AFSD/evaluation/eval_detection.py: the tail of compute_wilderness_impact :694-728 with utils_eval.interpolated_prec_rec
// :20-29, which run per class and threshold on the host over (nthr, K, N) arrays).  The rule is stated once in
// opental_amd/evaluation/table_wi.py (wi_reference / codes_reference); this file is its device form, otal_wilderness_impact.
//
// One workgroup of WI_TILE = 256 threads owns one (class, threshold) pair; pairs are independent, so nothing crosses a
// workgroup: no atomic, no scratch, no flag.  Every row r = 0 .. N-1 (the pass order: video by video, table row inside) gets
// its outcome from codes[t][r], pred_label[r] and gt_label (match.wi_outcome_codes), of which three kinds count here:
//   u   tp_u2u                                          -- steps the recall ratio, whatever the class;
//   a   tp_k2k, fp_k2k or fp_bg2k of THIS class         -- numerator and denominator of the precision ratio;
//   f   fp_u2k of THIS class                            -- denominator only.
// The rows are walked in chunks of WI_TILE, one row per thread, twice:
//   1. count    the totals of a, f and u, int32, no barrier inside the loop;
//   2. back     the chunks from the LAST to the first.  A chunk's counts give the cumulative counts at its start (those at
//               its end are carried: the totals for the last chunk), ballot prefixes give A_r, F_r, U_r inclusive of the row;
//               precision_r = A_r / ((A_r + F_r) + 1e-6); the envelope max over j >= r is a suffix maximum inside the wave
//               (shuffles), across the chunk's waves (LDS) and the carried maximum of the chunks behind; the rows where the
//               recall steps -- row 0 and the u rows -- contribute (recall_r - previous recall) * envelope_r with
//               recall_r = Kt / ((Kt + U) - U_r), the previous recall 0 for row 0 and Kt / ((Kt + U) - (U_r - 1)) otherwise.
// The closing step of interpolated_prec_rec (last recall -> 1) multiplies the appended precision 0 and adds +0.0: left out.
// The contributions of a chunk are summed by a butterfly inside each wave, the four waves' sums in wave order, and the chunks'
// sums from the last chunk to the first: an order fixed by WI_TILE and N alone, whatever the grid.  All of it is fp64 with
// IEEE division (the library is built with -ffp-contract=off and nothing here calls fma).
// Every barrier sits in a loop whose trip count comes from N alone, so all threads reach it.  A code outside -2 .. M-1 or a
// label outside 0 .. K is "no outcome" and gt_label is read only at a code inside 0 .. M-1: no input makes the kernel read out
// of bounds.
#include "common.h"

namespace {

constexpr int WI_TILE = OTAL_AP_TILE;
constexpr int WI_WAVES = WI_TILE / OTAL_WAVE;
static_assert(WI_TILE % OTAL_WAVE == 0 && WI_WAVES == 4, "the wave sums are added as ((s0 + s1) + s2) + s3");

enum { WI_NONE = 0, WI_U = 1, WI_A = 2, WI_F = 3 };

// match.wi_outcome_codes reduced to what the WI arithmetic reads; WI_A and WI_F belong to class lp - 1
__device__ __forceinline__ int wi_kind(int code, int lp, const int* __restrict__ gt_label, int M, int K) {
    if ((unsigned)lp > (unsigned)K) return WI_NONE;
    if (code == -1) return lp == 0 ? WI_NONE : WI_A;                    // fp_bg2u : fp_bg2k (folded into fp_k2k)
    if ((unsigned)code >= (unsigned)M) return WI_NONE;                  // -2, or out of range
    const int lg = gt_label[code];
    if ((unsigned)lg > (unsigned)K) return WI_NONE;
    if (lp == lg) return lg == 0 ? WI_U : WI_A;                         // tp_u2u : tp_k2k
    if (lg == 0) return WI_F;                                           // fp_u2k
    return lp == 0 ? WI_NONE : WI_A;                                    // fp_k2u : fp_k2k
}

__global__ __launch_bounds__(WI_TILE) void wilderness_impact_kernel(const int* __restrict__ codes,
                                                                    const int* __restrict__ pred_label,
                                                                    const int* __restrict__ gt_label, int n_known,
                                                                    int n_unknown, int N, int M, int K,
                                                                    double* __restrict__ out) {
    __shared__ int s_cnt[3][WI_WAVES];
    __shared__ double s_max[WI_WAVES];
    __shared__ double s_sum[WI_WAVES];
    const int c = blockIdx.x, t = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & (OTAL_WAVE - 1), wave = tid / OTAL_WAVE;
    const int nchunks = (N + WI_TILE - 1) / WI_TILE;
    if (nchunks == 0) {
        if (tid == 0) out[(size_t)t * K + c] = 0.0;
        return;
    }
    const int* row = codes + (size_t)t * N;
    const int mine_label = c + 1;
    const double kt = (double)n_known;
    const double total = (double)(n_known + n_unknown);

    // pass 1: the totals
    int na = 0, nf = 0, nu = 0;
    for (int r = tid; r < N; r += WI_TILE) {
        const int lp = pred_label[r];
        const int kind = wi_kind(row[r], lp, gt_label, M, K);
        na += (kind == WI_A && lp == mine_label) ? 1 : 0;
        nf += (kind == WI_F && lp == mine_label) ? 1 : 0;
        nu += (kind == WI_U) ? 1 : 0;
    }
    for (int off = OTAL_WAVE / 2; off > 0; off >>= 1) {
        na += __shfl_xor(na, off, OTAL_WAVE);
        nf += __shfl_xor(nf, off, OTAL_WAVE);
        nu += __shfl_xor(nu, off, OTAL_WAVE);
    }
    if (lane == 0) {
        s_cnt[0][wave] = na;
        s_cnt[1][wave] = nf;
        s_cnt[2][wave] = nu;
    }
    __syncthreads();
    int end_a = 0, end_f = 0, end_u = 0;            // the counts up to the end of the current chunk
    for (int w = 0; w < WI_WAVES; ++w) {
        end_a += s_cnt[0][w];
        end_f += s_cnt[1][w];
        end_u += s_cnt[2][w];
    }
    __syncthreads();                                // s_cnt is rewritten by the first chunk

    // pass 2: the chunks from the back
    double carry_max = 0.0;                         // the envelope of the rows behind the current chunk (the appended precision 0)
    double acc = 0.0;
    for (int k = nchunks - 1; k >= 0; --k) {
        const int r = k * WI_TILE + tid;
        const bool valid = r < N;
        bool is_a = false, is_f = false, is_u = false;
        if (valid) {
            const int lp = pred_label[r];
            const int kind = wi_kind(row[r], lp, gt_label, M, K);
            is_a = kind == WI_A && lp == mine_label;
            is_f = kind == WI_F && lp == mine_label;
            is_u = kind == WI_U;
        }
        const unsigned long long ba = __ballot(is_a), bf = __ballot(is_f), bu = __ballot(is_u);
        if (lane == 0) {
            s_cnt[0][wave] = __popcll(ba);
            s_cnt[1][wave] = __popcll(bf);
            s_cnt[2][wave] = __popcll(bu);
        }
        __syncthreads();
        int before_a = 0, before_f = 0, before_u = 0, total_a = 0, total_f = 0, total_u = 0;
        for (int w = 0; w < WI_WAVES; ++w) {
            const int xa = s_cnt[0][w], xf = s_cnt[1][w], xu = s_cnt[2][w];
            if (w < wave) {
                before_a += xa;
                before_f += xf;
                before_u += xu;
            }
            total_a += xa;
            total_f += xf;
            total_u += xu;
        }
        const int start_a = end_a - total_a, start_f = end_f - total_f, start_u = end_u - total_u;
        const unsigned long long upto = (2ull << lane) - 1ull;                              // inclusive of this row
        const int cum_a = start_a + before_a + __popcll(ba & upto);
        const int cum_f = start_f + before_f + __popcll(bf & upto);
        const int cum_u = start_u + before_u + __popcll(bu & upto);
        const double prec = valid ? (double)cum_a / (((double)cum_a + (double)cum_f) + 1e-6) : 0.0;
        double suf = prec;                          // max over the lanes >= this one
        for (int off = 1; off < OTAL_WAVE; off <<= 1) {
            const double o = __shfl_down(suf, off, OTAL_WAVE);
            if (lane + off < OTAL_WAVE && o > suf) suf = o;
        }
        if (lane == 0) s_max[wave] = suf;
        __syncthreads();
        double env = carry_max, chunk_max = carry_max;
        for (int w = 0; w < WI_WAVES; ++w) {
            const double x = s_max[w];
            if (w > wave && x > env) env = x;
            if (x > chunk_max) chunk_max = x;
        }
        if (suf > env) env = suf;
        double term = 0.0;
        if (valid && (r == 0 || is_u)) {
            const double rec = kt / (total - (double)cum_u);
            const double prev = r == 0 ? 0.0 : kt / (total - (double)(cum_u - 1));
            term = (rec - prev) * env;
        }
        for (int off = OTAL_WAVE / 2; off > 0; off >>= 1) term += __shfl_xor(term, off, OTAL_WAVE);
        if (lane == 0) s_sum[wave] = term;
        __syncthreads();
        acc += ((s_sum[0] + s_sum[1]) + s_sum[2]) + s_sum[3];
        carry_max = chunk_max;
        end_a = start_a;
        end_f = start_f;
        end_u = start_u;
        // s_cnt, s_max and s_sum are rewritten by the next chunk only after its own barriers: the reads above are behind one
    }
    if (tid == 0) out[(size_t)t * K + c] = acc;
}

}  // namespace

extern "C" int otal_wilderness_impact(const int* codes, const int* pred_label, const int* gt_label, int n_known, int n_unknown,
                                      int N, int M, int nthr, int K, double* out, void* stream) {
    if (!codes || !pred_label || !gt_label || !out) return OTAL_E_NULL;
    if (N < 0 || M < 0 || K < 1 || nthr < 1 || n_known < 1 || n_unknown < 0) return OTAL_E_SHAPE;
    // the host rule holds the ground-truth counts in float32: exact below 2^24, and so is their sum here
    if (nthr > 32 || N > OTAL_AP_MAX_CLASS_ROWS || n_known >= OTAL_WI_MAX_GT || n_unknown >= OTAL_WI_MAX_GT - n_known)
        return OTAL_E_UNSUPPORTED;
    hipLaunchKernelGGL(wilderness_impact_kernel, dim3(K, nthr), dim3(WI_TILE), 0, (hipStream_t)stream, codes, pred_label,
                       gt_label, n_known, n_unknown, N, M, K, out);
    return otal_launch_status();
}
