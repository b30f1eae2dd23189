// opental_amd/csrc/eval.hip -- the greedy prediction -> ground-truth matching of the detection evaluation on gfx950
// (AFSD/evaluation/eval_detection.py: compute_average_precision_detection :323-402 and split_results_by_gt :405-456, which
// walk every detection in Python).  The rule is stated once in opental_amd/evaluation/match.py (match_reference); this file
// is its device form, otal_eval_match.
//
// One wavefront (a workgroup of 64 threads) owns one group -- a video, or a (class, video) pair -- for ALL thresholds: the
// predictions of a group are a sequential chain (a ground truth can be taken once), groups are independent.  Lanes run over
// the group's ground truths in chunks of 64; the segments and one 32-bit word of taken-flags per ground truth (bit t =
// taken at threshold t, hence nthr <= 32) live in LDS.  Lane t < nthr also keeps the running best (tIoU, row) of threshold t,
// so that no per-threshold array is indexed dynamically.  Per prediction and chunk:
//   * every lane computes its fp64 tIoU in the operation order of utils_eval.segment_iou (plain IEEE division, the library
//     is built with -ffp-contract=off) and the word ge = {t : not (tIoU < thr_t)};
//   * for every threshold with a ballot of untaken candidates the wave walks the ballot's set bits in ascending lane order
//     and keeps the strictly larger tIoU: among equal tIoU the lowest row wins, inside a chunk and across chunks;
//   * predictions are the serial loop; 64 of them are loaded at once and handed out by v_readlane.
// A prediction that matches nothing is -1 where some ground truth lies below the threshold and -2 where all clear it (and
// are taken).  The non-finite tIoU of a zero-length prediction on a zero-length ground truth counts into *nonfinite.
//
// otal_eval_match_labeled is the same kernel instantiated with LABELED = true, the Wilderness-Impact pass's rule
// (match_labeled_reference; AFSD/evaluation/eval_detection.py: compute_wilderness_impact :604-728).  It differs in three
// places: the ground truths' labels sit in LDS next to the segments (24 bytes per ground truth) and the predictions' labels are
// loaded with the batch of 64; the winner's taken bit is set only where its label equals the prediction's (a true positive --
// a false positive leaves the ground truth open for later predictions); and every prediction's largest tIoU over the group's
// ground truths is written once (lane-wise running maximum over the chunks, then a wave reduction).
#include "common.h"

#include <math.h>

namespace {

constexpr int EV_CAP = OTAL_EVAL_MAX_GT;      // ground truths of one group that fit the LDS of its wave (20 or 24 bytes each)
static_assert(EV_CAP * (sizeof(double2) + sizeof(unsigned) + sizeof(int)) <= 64 * 1024, "one group's ground truths in LDS");

__device__ __forceinline__ double readlane_f64(double v, int lane) {      // `lane` is wave-uniform
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
    return __hiloint2double(hi, lo);
}

// the largest of the lanes' values (finite or -inf: a non-finite tIoU discards the whole result anyway)
__device__ __forceinline__ double wave_max_f64(double v) {
    for (int off = OTAL_WAVE / 2; off > 0; off >>= 1) {
        const double o = __shfl_xor(v, off, OTAL_WAVE);
        v = o > v ? o : v;
    }
    return v;
}

// LABELED: pred_label (N), gt_label (M) and max_tiou (N) are read / written; otherwise they are not touched.
template <bool LABELED>
__global__ __launch_bounds__(OTAL_WAVE) void eval_match_kernel(const double2* __restrict__ pred_seg,
                                                               const int* __restrict__ pred_label,
                                                               const int* __restrict__ pred_start,
                                                               const double2* __restrict__ gt_seg,
                                                               const int* __restrict__ gt_label,
                                                               const int* __restrict__ gt_start,
                                                               const double* __restrict__ thresholds, int ngroups, int nthr,
                                                               int* __restrict__ out, double* __restrict__ max_tiou,
                                                               int* __restrict__ nonfinite) {
    __shared__ double2 s_seg[EV_CAP];
    __shared__ unsigned s_taken[EV_CAP];
    __shared__ int s_label[LABELED ? EV_CAP : 1];
    const int g = blockIdx.x, lane = threadIdx.x;
    const int p0 = pred_start[g], p1 = pred_start[g + 1];
    if (p1 <= p0) return;
    const size_t N = (size_t)pred_start[ngroups];
    const int g0 = gt_start[g], m = gt_start[g + 1] - g0;
    if (m <= 0 || m > EV_CAP) {
        // no ground truth: every prediction is -1.  Too many for one wave's LDS: the same, and the counter tells the caller
        // that this result is not the rule's.
        for (int t = 0; t < nthr; ++t)
            for (int i = p0 + lane; i < p1; i += OTAL_WAVE) out[(size_t)t * N + i] = -1;
        if (LABELED)
            for (int i = p0 + lane; i < p1; i += OTAL_WAVE) max_tiou[i] = 0.0;
        if (m > EV_CAP && lane == 0) atomicAdd(nonfinite, 1);
        return;
    }
    for (int j = lane; j < m; j += OTAL_WAVE) {
        s_seg[j] = gt_seg[g0 + j];
        s_taken[j] = 0u;
        if (LABELED) s_label[j] = gt_label[g0 + j];
    }
    __syncthreads();
    const double mythr = lane < nthr ? thresholds[lane] : 0.0;
    const unsigned full = nthr >= 32 ? 0xffffffffu : (1u << nthr) - 1u;
    const int nchunks = (m + OTAL_WAVE - 1) / OTAL_WAVE;
    int nf = 0;
    for (int ib = p0; ib < p1; ib += OTAL_WAVE) {
        const int nb = min(OTAL_WAVE, p1 - ib);
        const double2 bp = pred_seg[min(ib + lane, p1 - 1)];
        const int blabel = LABELED ? pred_label[min(ib + lane, p1 - 1)] : 0;
        for (int k = 0; k < nb; ++k) {
            const double ps = readlane_f64(bp.x, k), pe = readlane_f64(bp.y, k);
            const int plabel = __builtin_amdgcn_readlane(blabel, k);
            double bestv = -INFINITY;       // lane t: best untaken candidate of threshold t so far
            int bestrow = -1;
            unsigned below = 0u;            // bit t: this lane saw a ground truth with tIoU < thr_t
            double top = -INFINITY;         // LABELED: this lane's largest tIoU over the chunks
            for (int c = 0; c < nchunks; ++c) {
                const int j = c * OTAL_WAVE + lane;
                const bool valid = j < m;
                const double2 gs = s_seg[min(j, m - 1)];
                const unsigned taken = s_taken[min(j, m - 1)];
                // utils_eval.segment_iou, operation by operation
                const double tt1 = fmax(ps, gs.x), tt2 = fmin(pe, gs.y);
                const double inter = fmax(tt2 - tt1, 0.0);
                const double uni = ((gs.y - gs.x) + (pe - ps)) - inter;
                const double tiou = inter / uni;
                unsigned ge = 0u;
                for (int t = 0; t < nthr; ++t)
                    if (!(tiou < readlane_f64(mythr, t))) ge |= 1u << t;
                const unsigned avail = valid ? ge & ~taken : 0u;
                if (valid) below |= ~ge & full;
                if (LABELED && valid && tiou > top) top = tiou;
                nf += __popcll(__ballot(valid && !isfinite(tiou)));
                if (__ballot(avail != 0u) == 0ull) continue;
                for (int t = 0; t < nthr; ++t) {
                    unsigned long long cand = __ballot((avail >> t) & 1u);
                    if (cand == 0ull) continue;
                    double bv = -INFINITY;
                    int bl = -1;
                    while (cand) {
                        const int b = __ffsll((long long)cand) - 1;
                        cand &= cand - 1ull;
                        const double v = readlane_f64(tiou, b);
                        if (v > bv) { bv = v; bl = b; }
                    }
                    if (lane == t && bl >= 0 && bv > bestv) {
                        bestv = bv;
                        bestrow = g0 + c * OTAL_WAVE + bl;
                    }
                }
            }
            int res = bestrow;
            unsigned long long open = __ballot(lane < nthr && bestrow < 0);
            while (open) {
                const int t = __ffsll((long long)open) - 1;
                open &= open - 1ull;
                const bool any_below = __ballot((below >> t) & 1u) != 0ull;
                if (lane == t) res = any_below ? -1 : -2;
            }
            if (lane < nthr) {
                out[(size_t)lane * N + ib + k] = res;
                // LABELED: only a true positive takes its ground truth
                const bool take = bestrow >= 0 && (!LABELED || s_label[max(bestrow - g0, 0)] == plabel);
                if (take) atomicOr(&s_taken[bestrow - g0], 1u << lane);
            }
            if (LABELED) {
                top = wave_max_f64(top);
                if (lane == 0) max_tiou[ib + k] = top;
            }
            __syncthreads();        // one wave: orders the LDS flag update before the next prediction's reads
        }
    }
    if (nf != 0 && lane == 0) atomicAdd(nonfinite, nf);
}

}  // namespace

extern "C" int otal_eval_match(const double* pred_seg, const int* pred_start, const double* gt_seg, const int* gt_start,
                               const double* thresholds, int ngroups, int nthr, int* out, int* nonfinite, void* stream) {
    if (!pred_seg || !pred_start || !gt_seg || !gt_start || !thresholds || !out || !nonfinite) return OTAL_E_NULL;
    if (ngroups < 0 || nthr < 1) return OTAL_E_SHAPE;
    if (nthr > 32 || ((uintptr_t)pred_seg & 15) || ((uintptr_t)gt_seg & 15)) return OTAL_E_UNSUPPORTED;
    if (ngroups == 0) return 0;
    hipLaunchKernelGGL(eval_match_kernel<false>, dim3(ngroups), dim3(OTAL_WAVE), 0, (hipStream_t)stream,
                       reinterpret_cast<const double2*>(pred_seg), nullptr, pred_start,
                       reinterpret_cast<const double2*>(gt_seg), nullptr, gt_start, thresholds, ngroups, nthr, out, nullptr,
                       nonfinite);
    return otal_launch_status();
}

extern "C" int otal_eval_match_labeled(const double* pred_seg, const int* pred_label, const int* pred_start,
                                       const double* gt_seg, const int* gt_label, const int* gt_start,
                                       const double* thresholds, int ngroups, int nthr, int* out, double* max_tiou,
                                       int* nonfinite, void* stream) {
    if (!pred_seg || !pred_label || !pred_start || !gt_seg || !gt_label || !gt_start || !thresholds || !out || !max_tiou ||
        !nonfinite)
        return OTAL_E_NULL;
    if (ngroups < 0 || nthr < 1) return OTAL_E_SHAPE;
    if (nthr > 32 || ((uintptr_t)pred_seg & 15) || ((uintptr_t)gt_seg & 15)) return OTAL_E_UNSUPPORTED;
    if (ngroups == 0) return 0;
    hipLaunchKernelGGL(eval_match_kernel<true>, dim3(ngroups), dim3(OTAL_WAVE), 0, (hipStream_t)stream,
                       reinterpret_cast<const double2*>(pred_seg), pred_label, pred_start,
                       reinterpret_cast<const double2*>(gt_seg), gt_label, gt_start, thresholds, ngroups, nthr, out, max_tiou,
                       nonfinite);
    return otal_launch_status();
}
