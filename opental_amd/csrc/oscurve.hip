// opental_amd/csrc/oscurve.hip -- AUROC, AUPR, FAR@95 and OSDR per tIoU threshold from the matched detections of the split pass
// on gfx950 (AFSD/evaluation/eval_detection.py: compute_auc_scores :459-491 and compute_osdr_scores :494-510 with the curve
// functions of utils_eval, which run per threshold on the host).  The rule is stated once in
// opental_amd/evaluation/table_open.py (open_reference); this file is its device form, otal_open_set_curves.
//
// One workgroup of OS_TILE = 256 threads owns one threshold; thresholds are independent, so nothing crosses a workgroup: no
// atomic, no scratch, no flag.  A threshold's list is the entries before its first empty slot (flags < 0), n <= M of them, in
// ascending known-ness, that is descending ood = 1.0 - known.  Two reductions find n, then P (unknown entries) and the number
// of correct entries; then the list is walked from the front in chunks of OS_TILE, one entry per thread:
//   counts   a ballot prefix gives the unknown / correct entries before every entry, the chunks before are carried;
//   ends     an entry ends its tie group where the next entry's ood differs.  A scan hands every entry the last TWO group ends
//            before it as (position, tps) pairs -- fps = position + 1 - tps.  At a group end that gives the AUPR term
//            (recall - previous recall) * tps / (position + 1), and, with this end's own counts, roc_curve's drop_intermediate
//            predicate for the PREVIOUS end: kept when it is the first one or a second difference of fps or tps is not 0;
//   kept     a second scan hands every entry the last kept end before it; where an entry decided that the previous end A is
//            kept it adds the trapezoid from the kept end before A (or the prepended (0, 0)) to A and offers A to the running
//            argmin of |tpr - 0.95| (the lowest position among equal values);
//   cuts     entry j adds the OSDR trapezoid between the curve points j and j + 1 of (1, 1), cut 0 .. cut n-2, (0, 0), with
//            the suffix counts total - prefix.
// The last group end is always kept and has no entry behind it: its trapezoid and its offer come after the loop.
// A chunk's terms are summed by a butterfly inside each wave, the four waves' sums in wave order, the chunks in order, the last
// ROC point last: an order fixed by OS_TILE and n alone.  All of it is fp64 with IEEE division (the library is built with
// -ffp-contract=off and nothing here calls fma).  Every barrier sits outside the loops or in the chunk loop, whose trip count
// comes from n, which all threads read from the same reduction.  Every index is below n <= M: no input makes the kernel read
// out of bounds.
#include "common.h"

#include <limits.h>
#include <math.h>

namespace {

constexpr int OS_TILE = OTAL_AP_TILE;
constexpr int OS_WAVES = OS_TILE / OTAL_WAVE;
static_assert(OS_TILE % OTAL_WAVE == 0 && OS_WAVES == 4, "the wave sums are added as ((s0 + s1) + s2) + s3");

typedef long long pt_t;     // a group end: (position << 32) | tps, growing with the position; -1: none

__device__ __forceinline__ pt_t make_pt(int pos, int tps) { return ((pt_t)pos << 32) | (pt_t)(unsigned)tps; }
__device__ __forceinline__ long long pt_pos(pt_t p) { return p >> 32; }
__device__ __forceinline__ long long pt_tps(pt_t p) { return p & 0xffffffffll; }

struct Last2 {              // the most recent group end and the one before it
    pt_t a, b;
};
__device__ __forceinline__ Last2 join(Last2 l, Last2 r) {       // l's entries come before r's
    if (r.a < 0) return l;
    if (r.b < 0) return Last2{r.a, l.a};
    return r;
}

__device__ __forceinline__ int wave_sum(int v) {
    for (int off = OTAL_WAVE / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, OTAL_WAVE);
    return v;
}
__device__ __forceinline__ double wave_sum(double v) {
    for (int off = OTAL_WAVE / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, OTAL_WAVE);
    return v;
}

__global__ __launch_bounds__(OS_TILE) void open_set_curves_kernel(const double* __restrict__ known,
                                                                  const int* __restrict__ flags, int M,
                                                                  double* __restrict__ out) {
    __shared__ int s_cnt[2][OS_WAVES];
    __shared__ pt_t s_a[OS_WAVES], s_b[OS_WAVES], s_kept[OS_WAVES];
    __shared__ double s_sum[3][OS_WAVES];
    __shared__ double s_d[OS_WAVES];
    __shared__ long long s_dpos[OS_WAVES], s_dfps[OS_WAVES];
    const int t = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & (OTAL_WAVE - 1), wave = tid / OTAL_WAVE;
    const double* kn = known + (size_t)t * M;
    const int* fl = flags + (size_t)t * M;

    // the list's length: the first empty slot
    int first = M;
    for (int i = tid; i < M; i += OS_TILE)
        if (fl[i] < 0) first = min(first, i);
    for (int off = OTAL_WAVE / 2; off > 0; off >>= 1) first = min(first, __shfl_xor(first, off, OTAL_WAVE));
    if (lane == 0) s_cnt[0][wave] = first;
    __syncthreads();
    int n = M;
    for (int w = 0; w < OS_WAVES; ++w) n = min(n, s_cnt[0][w]);
    __syncthreads();                    // s_cnt is rewritten below
    if (n <= 0) {                       // the same n in every thread
        if (tid < 4) out[(size_t)t * 4 + tid] = 0.0;
        return;
    }

    // the unknown and the correct entries of the list
    int mu = 0, mc = 0;
    for (int i = tid; i < n; i += OS_TILE) {
        const int f = fl[i];
        mu += f & 1;
        mc += (f & 3) == 2 ? 1 : 0;
    }
    mu = wave_sum(mu);
    mc = wave_sum(mc);
    if (lane == 0) {
        s_cnt[0][wave] = mu;
        s_cnt[1][wave] = mc;
    }
    __syncthreads();
    int P = 0, C = 0;
    for (int w = 0; w < OS_WAVES; ++w) {
        P += s_cnt[0][w];
        C += s_cnt[1][w];
    }
    __syncthreads();                    // s_cnt is rewritten by the first chunk
    const int Q = n - P;
    const double Pd = (double)P, Qd = (double)Q;
    const bool both = P > 0 && Q > 0;

    int carry_u = 0, carry_c = 0;       // unknown / correct entries of the chunks before
    Last2 carry_ends{-1, -1};           // the last two group ends of the chunks before
    pt_t carry_kept = -1;               // the last kept end decided in the chunks before
    // the running argmin starts at the prepended point (0, 0)
    double best_d = fabs(0.0 / Pd - 0.95);
    long long best_fps = 0;
    double acc_roc = 0.0, acc_pr = 0.0, acc_os = 0.0;
    const int nchunks = (n + OS_TILE - 1) / OS_TILE;
    for (int k = 0; k < nchunks; ++k) {
        const int i = k * OS_TILE + tid;
        const bool valid = i < n;
        const int f = valid ? fl[i] : 0;
        const bool u = valid && (f & 1) != 0;
        const bool c = valid && (f & 3) == 2;
        bool end = false;
        if (valid) end = i == n - 1 || (1.0 - kn[i + 1]) != (1.0 - kn[i]);
        const int uprev = (valid && i > 0) ? (fl[i - 1] & 1) : 0;

        // counts
        const unsigned long long bu = __ballot(u), bc = __ballot(c);
        if (lane == 0) {
            s_cnt[0][wave] = __popcll(bu);
            s_cnt[1][wave] = __popcll(bc);
        }
        __syncthreads();
        int ubefore = 0, cbefore = 0, utot = 0, ctot = 0;
        for (int w = 0; w < OS_WAVES; ++w) {
            const int xu = s_cnt[0][w], xc = s_cnt[1][w];
            if (w < wave) {
                ubefore += xu;
                cbefore += xc;
            }
            utot += xu;
            ctot += xc;
        }
        const unsigned long long below = (1ull << lane) - 1ull;
        const int u_ex = carry_u + ubefore + __popcll(bu & below);      // unknown entries before this one
        const int c_ex = carry_c + cbefore + __popcll(bc & below);
        const int u_in = u_ex + (u ? 1 : 0);

        // ends: the last two group ends before this entry
        Last2 x{end ? make_pt(i, u_in) : (pt_t)-1, (pt_t)-1};
        for (int off = 1; off < OTAL_WAVE; off <<= 1) {
            const Last2 o{__shfl_up(x.a, off, OTAL_WAVE), __shfl_up(x.b, off, OTAL_WAVE)};
            if (lane >= off) x = join(o, x);
        }
        Last2 ex{__shfl_up(x.a, 1, OTAL_WAVE), __shfl_up(x.b, 1, OTAL_WAVE)};
        if (lane == 0) ex = Last2{-1, -1};
        if (lane == OTAL_WAVE - 1) {
            s_a[wave] = x.a;
            s_b[wave] = x.b;
        }
        __syncthreads();
        Last2 pre = carry_ends, all = carry_ends;
        for (int w = 0; w < OS_WAVES; ++w) {
            const Last2 y{s_a[w], s_b[w]};
            if (w < wave) pre = join(pre, y);
            all = join(all, y);
        }
        const Last2 prev = join(pre, ex);

        double t_pr = 0.0;
        pt_t kept = -1;
        if (end) {
            const double r = P > 0 ? (double)u_in / Pd : 1.0;
            const double rp = prev.a < 0 ? 0.0 : (P > 0 ? (double)pt_tps(prev.a) / Pd : 1.0);
            t_pr = (r - rp) * ((double)u_in / (double)(i + 1));
            if (prev.a >= 0) {          // does drop_intermediate keep the previous end A, between B and this end?
                bool keep = prev.b < 0;
                if (!keep) {
                    const long long tA = pt_tps(prev.a), tB = pt_tps(prev.b), tC = u_in;
                    const long long fA = pt_pos(prev.a) + 1 - tA, fB = pt_pos(prev.b) + 1 - tB, fC = (long long)i + 1 - tC;
                    keep = (fB - 2 * fA + fC) != 0 || (tB - 2 * tA + tC) != 0;
                }
                if (keep) kept = prev.a;
            }
        }

        // kept: the last kept end before the one this entry decided
        pt_t y = kept;
        for (int off = 1; off < OTAL_WAVE; off <<= 1) {
            const pt_t o = __shfl_up(y, off, OTAL_WAVE);
            if (lane >= off && o > y) y = o;
        }
        pt_t yex = __shfl_up(y, 1, OTAL_WAVE);
        if (lane == 0) yex = -1;
        if (lane == OTAL_WAVE - 1) s_kept[wave] = y;
        __syncthreads();
        pt_t kpre = carry_kept, kall = carry_kept;
        for (int w = 0; w < OS_WAVES; ++w) {
            const pt_t z = s_kept[w];
            if (w < wave && z > kpre) kpre = z;
            if (z > kall) kall = z;
        }
        if (yex > kpre) kpre = yex;

        double t_roc = 0.0, d = INFINITY;
        long long dpos = LLONG_MAX, dfps = 0;
        if (kept >= 0 && both) {
            const long long tA = pt_tps(kept), fA = pt_pos(kept) + 1 - tA;
            const long long tK = kpre < 0 ? 0 : pt_tps(kpre), fK = kpre < 0 ? 0 : pt_pos(kpre) + 1 - tK;
            const double tprA = (double)tA / Pd;
            t_roc = ((double)fA / Qd - (double)fK / Qd) * (tprA + (double)tK / Pd) / 2.0;
            d = fabs(tprA - 0.95);
            dpos = pt_pos(kept);
            dfps = fA;
        }

        // cuts: the trapezoid between the curve points i and i + 1 of (1, 1), cut 0 .. cut n-2, (0, 0)
        double t_os = 0.0;
        if (valid) {
            double f0 = 1.0, c0 = 1.0, f1 = 0.0, c1 = 0.0;
            if (i > 0) {                // cut i - 1
                f0 = P > 0 ? (double)(P - u_ex + uprev) / Pd : 0.0;
                c0 = Q > 0 ? (double)(C - c_ex) / Qd : 1.0;
            }
            if (i < n - 1) {            // cut i
                f1 = P > 0 ? (double)(P - u_ex) / Pd : 0.0;
                c1 = Q > 0 ? (double)(C - c_ex - (c ? 1 : 0)) / Qd : 1.0;
            }
            t_os = (f0 - f1) * (c0 + c1) / 2.0;
        }

        t_roc = wave_sum(t_roc);
        t_pr = wave_sum(t_pr);
        t_os = wave_sum(t_os);
        for (int off = OTAL_WAVE / 2; off > 0; off >>= 1) {
            const double od = __shfl_xor(d, off, OTAL_WAVE);
            const long long op = __shfl_xor(dpos, off, OTAL_WAVE), of = __shfl_xor(dfps, off, OTAL_WAVE);
            if (od < d || (od == d && op < dpos)) {
                d = od;
                dpos = op;
                dfps = of;
            }
        }
        if (lane == 0) {
            s_sum[0][wave] = t_roc;
            s_sum[1][wave] = t_pr;
            s_sum[2][wave] = t_os;
            s_d[wave] = d;
            s_dpos[wave] = dpos;
            s_dfps[wave] = dfps;
        }
        __syncthreads();
        acc_roc += ((s_sum[0][0] + s_sum[0][1]) + s_sum[0][2]) + s_sum[0][3];
        acc_pr += ((s_sum[1][0] + s_sum[1][1]) + s_sum[1][2]) + s_sum[1][3];
        acc_os += ((s_sum[2][0] + s_sum[2][1]) + s_sum[2][2]) + s_sum[2][3];
        for (int w = 0; w < OS_WAVES; ++w)      // ascending positions: a strict comparison keeps the lowest among equal values
            if (s_d[w] < best_d) {
                best_d = s_d[w];
                best_fps = s_dfps[w];
            }
        carry_u += utot;
        carry_c += ctot;
        carry_ends = all;
        carry_kept = kall;
        // every shared array is rewritten by the next chunk only behind one of its barriers: the reads above are before it
    }

    // the last group end (position n - 1, tps = P, fps = Q) is always kept
    if (both) {
        const long long tK = carry_kept < 0 ? 0 : pt_tps(carry_kept), fK = carry_kept < 0 ? 0 : pt_pos(carry_kept) + 1 - tK;
        const double tprL = Pd / Pd;
        acc_roc += (Qd / Qd - (double)fK / Qd) * (tprL + (double)tK / Pd) / 2.0;
        if (fabs(tprL - 0.95) < best_d) best_fps = Q;
    }
    if (tid == 0) {
        double* o = out + (size_t)t * 4;
        o[0] = both ? acc_roc : 0.0;
        o[1] = acc_pr;
        o[2] = P == 0 ? 0.0 : (Q == 0 ? (double)NAN : (double)best_fps / Qd);
        o[3] = acc_os;
    }
}

}  // namespace

extern "C" int otal_open_set_curves(const double* known, const int* flags, int M, int nthr, double* out, void* stream) {
    if (!known || !flags || !out) return OTAL_E_NULL;
    if (M < 0 || nthr < 1) return OTAL_E_SHAPE;
    if (nthr > 32 || M > OTAL_AP_MAX_CLASS_ROWS) return OTAL_E_UNSUPPORTED;
    hipLaunchKernelGGL(open_set_curves_kernel, dim3(nthr), dim3(OS_TILE), 0, (hipStream_t)stream, known, flags, M, out);
    return otal_launch_status();
}
