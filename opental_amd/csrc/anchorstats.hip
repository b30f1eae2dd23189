// opental_amd/csrc/anchorstats.hip -- the anchor diagnostics of a trained THUMOS14 detector on gfx950: per anchor and stage
// (coarse / refined) the matched label, one score and the EDL gradient 1/alpha_y - C/S, and their histograms
// (reference: get_matched_targets + get_result + the group split, experiments/analyze_actionness.py:226-339; grad_edl and the
// bins of plot_grad_density, experiments/analyze_gradnorm.py:173-189,:248-262).  The rule is stated once in
// opental_amd/common/anchor_stats.py (anchor_stats_reference); this file is its device form, otal_anchor_stats.
//
// One launch on the caller's stream, no allocation, no synchronisation.  One workgroup of 256 threads per sample, the K
// anchors strided over the threads (K is not bounded by the workgroup).  A thread does everything of its anchor: the matching
// loop over the G ground truths (the operations and their order of detection_loss_kernel's phase 1, csrc/loss.hip, so the
// labels are the loss's), the IoU test, and per stage ONE pass over the C logits (sum, label column, running maximum), the
// score and the gradient.  Histograms are counted in LDS with integer adds; after a barrier the workgroup makes one 64-bit
// integer add to the global array per non-empty bin.  Counts are integers: the result does not depend on the order of the
// adds and is identical from run to run, and the global arrays accumulate over launches.
// The library is built with -ffp-contract=off and nothing here calls fma.
#include "common.h"
#include "evidence.h"

namespace {

constexpr int AS_THREADS = 256;
constexpr int AS_MAX_LDS_BYTES = 64 * 1024;                     // dynamic LDS a launch may ask for without an opt-in
constexpr float AS_EPS = 1.1920928955078125e-07f;               // torch.finfo(float32).eps
constexpr int AS_GROUPS = 3;                                    // known, unknown, background

struct AnchorStatsArgs {
    const float *loc, *conf, *prop_conf, *center, *act, *prop_act, *priors, *gt;
    const unsigned char* gvalid;
    int K, C, G;
    float clip, overlap;
    int os_head, n_known, target, score_bins, grad_bins;
    int evidence;                                               // EV instance (otal_anchor_stats_ev): the kind of csrc/evidence.h
    unsigned long long *hist_score, *hist_grad;
    int* label;
    float *value, *grad;
};

__device__ __forceinline__ float as_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

// the bin of a gradient length (plot_grad_density, analyze_gradnorm.py:250-262): edges[b] <= g < edges[b + 1] with
// edges[b] = b / num_bins in double rounded to float and 1e-6 added to the last one; -1: none.  The rule of ghm_bin in
// csrc/loss.hip (reweight 2), restated here because that one lives in the loss's translation unit.
__device__ int as_grad_bin(float g, int num_bins) {
    auto edge = [&](int b) { return (float)((double)b / (double)num_bins + (b == num_bins ? 1e-6 : 0.0)); };
    if (!(g >= 0.f)) return -1;                                 // NaN
    int b = min(max((int)fminf(g * (float)num_bins, (float)num_bins), 0), num_bins - 1);
    if (g < edge(b)) --b;
    else if (g >= edge(b + 1)) ++b;
    return (b >= 0 && b < num_bins && g >= edge(b) && g < edge(b + 1)) ? b : -1;
}

// EV: alpha = evidence(z) + 1 with the caller's evidence function (grad_edl with the network's evidence, analyze_gradnorm.py:
// 164-184); false is the exp code as it was.
template <bool EV>
__global__ __launch_bounds__(AS_THREADS) void anchor_stats_kernel(const AnchorStatsArgs a) {
    extern __shared__ unsigned int s_hist[];        // [2][3][score_bins] then [2][grad_bins]
    const int b = blockIdx.x, t = threadIdx.x;
    const int nscore = 2 * AS_GROUPS * a.score_bins, ngrad = 2 * a.grad_bins;
    for (int e = t; e < nscore + ngrad; e += AS_THREADS) s_hist[e] = 0u;
    __syncthreads();
    unsigned int* s_score = s_hist;
    unsigned int* s_grad = s_hist + nscore;
    const int K = a.K, C = a.C, G = a.G;
    const float* gtb = a.gt + (size_t)b * G * 3;
    const unsigned char* gvb = a.gvalid + (size_t)b * G;

    for (int k = t; k < K; k += AS_THREADS) {
        const size_t i = (size_t)b * K + k;
        // ---- matching (get_matched_targets; detection_loss_kernel phase 1)
        const float c = a.priors[k];
        const float big = a.clip * 2.f;
        float best_area = 0.f;
        int best = 0;
        for (int g = 0; g < G; ++g) {
            const float left = (c - gtb[g * 3]) * a.clip, right = (gtb[g * 3 + 1] - c) * a.clip;
            float area = left + right;
            if (left < 0.f || right < 0.f || !gvb[g]) area = big;
            if (g == 0 || area < best_area) { best_area = area; best = g; }     // first minimum, like torch.min
        }
        const float g0 = gtb[best * 3], g1 = gtb[best * 3 + 1], lab = gtb[best * 3 + 2];
        const float lt0 = (c - g0) * a.clip, lt1 = (g1 - c) * a.clip;
        int y[2];
        y[0] = best_area >= big ? 0 : (int)lab;
        const float p0 = a.loc[2 * i], p1 = a.loc[2 * i + 1];
        const float inter = fminf(p0, lt0) + fminf(p1, lt1);
        const float uni = (lt0 + lt1) + (p0 + p1) - inter;
        const float iou = inter / fmaxf(uni, AS_EPS);
        y[1] = iou < a.overlap ? 0 : y[0];

        const float ct = a.target == 2 ? as_sigmoid(a.center[i]) : 0.f;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            // ---- one pass over the logits: S, alpha at the label's column, the largest alpha
            const float* z = (s == 0 ? a.conf : a.prop_conf) + i * C;
            const int col = a.os_head ? y[s] - 1 : y[s];                        // os_head: rows 1..C count, at column y - 1
            float S = 0.f, amax = 0.f, ay = 1.f;
            for (int q = 0; q < C; ++q) {
                float al;
                if constexpr (EV) al = otal_ev::alpha(z[q], a.evidence);
                else al = expf(fminf(fmaxf(z[q], -10.f), 10.f)) + 1.f;
                S += al;
                amax = fmaxf(amax, al);
                if (q == col) ay = al;
            }
            const float u = (float)C / S;
            const float an = a.act ? as_sigmoid((s == 0 ? a.act : a.prop_act)[i]) : 0.f;
            float v;
            switch (a.target) {
            case 0: v = u; break;                                               // uncertainty
            case 1: v = an; break;                                              // actionness
            case 2: v = amax / S * ct; if (a.os_head) v = v * an; break;        // confidence: max_k of a monotone map of alpha_k
            case 3: v = u * an; break;                                          // uncertainty_actionness
            default: v = 0.5f * (an + 1.0f) * u; break;                         // half_au
            }
            const bool counts = col >= 0 && col < C;
            const float gr = counts ? 1.f / ay - u : 0.f;
            if (a.label) a.label[2 * i + s] = y[s];
            if (a.value) a.value[2 * i + s] = v;
            if (a.grad) a.grad[2 * i + s] = gr;
            if (v == v) {                                                       // a NaN score is counted nowhere
                const int grp = y[s] == 0 ? 2 : (y[s] <= a.n_known ? 0 : 1);
                const float scaled = fminf(fmaxf(floorf(v * (float)a.score_bins), 0.f), (float)(a.score_bins - 1));
                atomicAdd(&s_score[(s * AS_GROUPS + grp) * a.score_bins + (int)scaled], 1u);
            }
            if (counts) {
                const int gb = as_grad_bin(fabsf(gr), a.grad_bins);
                if (gb >= 0) atomicAdd(&s_grad[s * a.grad_bins + gb], 1u);
            }
        }
    }
    __syncthreads();
    for (int e = t; e < nscore; e += AS_THREADS)
        if (s_score[e]) atomicAdd(&a.hist_score[e], (unsigned long long)s_score[e]);
    for (int e = t; e < ngrad; e += AS_THREADS)
        if (s_grad[e]) atomicAdd(&a.hist_grad[e], (unsigned long long)s_grad[e]);
}

int anchor_stats_entry(const float* loc, const float* conf, const float* prop_conf, const float* center,
                                 const float* act, const float* prop_act, const float* priors, const float* gt,
                                 const unsigned char* gvalid, int B, int K, int C, int G, float clip_length, float overlap_thresh,
                                 int os_head, int n_known, int target, int score_bins, int grad_bins, long long* hist_score,
                                 long long* hist_grad, int* label, float* value, float* grad, bool ev, int evidence,
                                 void* stream) {
    if (!loc || !conf || !prop_conf || !center || !priors || !gt || !gvalid || !hist_score || !hist_grad) return OTAL_E_NULL;
    if (B < 1 || K < 1 || C < 1 || G < 1 || score_bins < 1 || grad_bins < 1) return OTAL_E_SHAPE;
    if (target < 0 || target > 4 || n_known < 1) return OTAL_E_UNSUPPORTED;
    if (ev && (evidence < 0 || evidence >= otal_ev::EV_KINDS)) return OTAL_E_UNSUPPORTED;
    const bool uses_act = target == 1 || target == 3 || target == 4 || (target == 2 && os_head);
    if (uses_act && (!act || !prop_act)) return OTAL_E_UNSUPPORTED;
    if ((act == nullptr) != (prop_act == nullptr)) return OTAL_E_UNSUPPORTED;
    const long long lds = 4ll * (2ll * AS_GROUPS * score_bins + 2ll * grad_bins);
    if (lds > AS_MAX_LDS_BYTES) return OTAL_E_UNSUPPORTED;                       // the histograms of a workgroup live in LDS
    AnchorStatsArgs a;
    a.loc = loc; a.conf = conf; a.prop_conf = prop_conf; a.center = center; a.act = act; a.prop_act = prop_act;
    a.priors = priors; a.gt = gt; a.gvalid = gvalid;
    a.K = K; a.C = C; a.G = G;
    a.clip = clip_length; a.overlap = overlap_thresh;
    a.os_head = os_head ? 1 : 0; a.n_known = n_known; a.target = target; a.score_bins = score_bins; a.grad_bins = grad_bins;
    a.hist_score = reinterpret_cast<unsigned long long*>(hist_score);
    a.hist_grad = reinterpret_cast<unsigned long long*>(hist_grad);
    a.label = label; a.value = value; a.grad = grad;
    a.evidence = evidence;
    if (ev) hipLaunchKernelGGL(anchor_stats_kernel<true>, dim3(B), dim3(AS_THREADS), (size_t)lds, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(anchor_stats_kernel<false>, dim3(B), dim3(AS_THREADS), (size_t)lds, (hipStream_t)stream, a);
    return otal_launch_status();
}

}  // namespace

extern "C" int otal_anchor_stats(const float* loc, const float* conf, const float* prop_conf, const float* center,
                                 const float* act, const float* prop_act, const float* priors, const float* gt,
                                 const unsigned char* gvalid, int B, int K, int C, int G, float clip_length, float overlap_thresh,
                                 int os_head, int n_known, int target, int score_bins, int grad_bins, long long* hist_score,
                                 long long* hist_grad, int* label, float* value, float* grad, void* stream) {
    return anchor_stats_entry(loc, conf, prop_conf, center, act, prop_act, priors, gt, gvalid, B, K, C, G, clip_length,
                              overlap_thresh, os_head, n_known, target, score_bins, grad_bins, hist_score, hist_grad, label, value,
                              grad, false, 0, stream);
}

// otal_anchor_stats with the network's evidence function (0 exp, 1 relu, 2 softplus): alpha_k = evidence(z_k) + 1 in S, in
// the scores and in the EDL gradient.  evidence 0 gives what otal_anchor_stats gives.
extern "C" int otal_anchor_stats_ev(const float* loc, const float* conf, const float* prop_conf, const float* center,
                                    const float* act, const float* prop_act, const float* priors, const float* gt,
                                    const unsigned char* gvalid, int B, int K, int C, int G, float clip_length,
                                    float overlap_thresh, int os_head, int n_known, int target, int score_bins, int grad_bins,
                                    long long* hist_score, long long* hist_grad, int* label, float* value, float* grad,
                                    int evidence, void* stream) {
    return anchor_stats_entry(loc, conf, prop_conf, center, act, prop_act, priors, gt, gvalid, B, K, C, G, clip_length,
                              overlap_thresh, os_head, n_known, target, score_bins, grad_bins, hist_score, hist_grad, label, value,
                              grad, true, evidence, stream);
}
