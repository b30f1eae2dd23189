// opental_amd/csrc/infer.hip -- inference post-processing of the OpenTAL detector on gfx950:
//   otal_decode_clips   : parse_output + decode_predictions + the per-class threshold test of
//                         `filtering` (AFSD/thumos14/test.py:79-162) for a batch of clips, one launch -- the OpenTAL
//                         head (Dirichlet scores x actionness);
//   otal_decode_clips_ex: the same with the score function (Dirichlet / softmax), the background class and the
//                         actionness heads chosen by the caller -- the closed-set Softmax and EDL baselines;
//   otal_decode_clips_ev: the same with the evidence function of the Dirichlet scores (exp / relu / softplus, csrc/evidence.h);
//   otal_decode_clips_2s: otal_decode_clips_ev on the average of two networks' raw maps (rgb + flow), taken in registers;
//   otal_softnms_classes: per (video, class) gather of the surviving candidates in the reference's
//                         order (clip-major, anchor-minor) followed by Gaussian Soft-NMS
//                         (softnms_v2, AFSD/common/segment_utils.py:128-162) -- one workgroup per
//                         (video, class), candidates resident in LDS for the whole greedy loop.
// The reference does all of this on the host: 15 boolean-mask kernels + syncs per clip, a .cpu()
// copy and a Python while-loop per class.  Here a whole batch of videos is two launches.
//
// Soft-NMS semantics kept bit for bit on the kept-index set: candidates with
// score >= thr are "undone"; each round takes the FIRST maximum among undone, marks it done, decays
// every other undone score by exp(-iou^2 / sigma) and drops those < thr; the loop stops when <= 1
// candidate is undone (so the last survivor is never kept) or top_k are done; rows come out in
// original index order with the decayed scores.  Latency-bound (min(top_k, N) dependent rounds), so
// the figure of merit is candidates/s, not bytes.
#include "common.h"
#include "evidence.h"

namespace {

constexpr int NMS_THREADS = 256;

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }

// The second network of a two-stream decode (otal_decode_clips_2s), by value in the kernel arguments; empty single-stream.
//   loc .. prop_act: the flow network's maps, laid out as the rgb network's (act / prop_act NULL with the rgb ones);
//   unct .. flow_prop_unct: BOTH networks' own uncertainty maps (clip, A), all four or none;
//   conf_sign: +1, or -1 for the GCPL decode (the averaged conf / prop_conf negated).
struct FlowMaps {
    const float *loc, *prop_loc, *conf, *prop_conf, *center, *act, *prop_act;
    const float *unct, *prop_unct, *flow_unct, *flow_prop_unct;
    float conf_sign;
};

// (a + b) / 2 as a FINISHED fp32 value: never contracted with the arithmetic that reads it, whatever -ffp-contract the file is
// built with (0.5f * w * prop + (a + b) * 0.5f as fma(a + b, 0.5f, 0.5f * w * prop) would round differently from the decode of
// the averaged map).  Halving is exact, so this is the fp32 sum of the two maps, halved: what (rgb + flow) / 2.0 gives in torch.
__device__ __forceinline__ float avg2(float a, float b) {
#pragma clang fp contract(off)
    const float s = a + b;
    return s * 0.5f;
}

// The one loader of the decode kernel's map values: element j of the map, or of the two networks' averaged map.
template <bool TWO>
__device__ __forceinline__ float ld_map(const float* a, const float* b, size_t j) {
    if constexpr (TWO) return avg2(a[j], b[j]);
    else return a[j];
}

// one workgroup per clip; A anchors, K logits per anchor.  Outputs: seg (clip,A,2) seconds; score (clip,K-first_class,A);
// unct (clip,A); actn (clip,A); flag (clip,K-first_class,A) uint8.
// SOFTMAX false: Dirichlet mean with exp evidence (BDNet.py DirichletLayer); true: softmax, exp(z - max) / sum (nn.Softmax).
// first_class 1 drops class 0 (the closed-set background) from score / flag.  act / prop_act NULL (no actionness heads):
// no actionness factor and flag = score > conf_thresh.  unct / actn NULL: not written; with SOFTMAX or without act the
// absent quantity is written as 0.  EV (SOFTMAX false): alpha = evidence(z) + 1 of csrc/evidence.h with the caller's evidence kind;
// false is the exp code as it was.
// TWO: every map value is ld_map's average of the map and its FlowMaps partner (conf / prop_conf times conf_sign), and with the
// four uncertainty maps unct = ((unct + flow_unct) / 2 + (prop_unct + flow_prop_unct) / 2) / 2 instead of the derived value.
template <bool SOFTMAX, bool EV = false, bool TWO = false>
__global__ __launch_bounds__(128) void decode_clips_kernel(
        const float* __restrict__ loc, const float* __restrict__ prop_loc, const float* __restrict__ priors,
        const float* __restrict__ conf, const float* __restrict__ prop_conf, const float* __restrict__ center,
        const float* __restrict__ act, const float* __restrict__ prop_act, const float* __restrict__ offsets,
        const float* __restrict__ fps, float* __restrict__ seg, float* __restrict__ score, float* __restrict__ unct,
        float* __restrict__ actn, unsigned char* __restrict__ flag, int A, int K, float clip_length,
        float conf_thresh, int first_class, int evidence, const FlowMaps f) {
    const int c = blockIdx.x;
    const int KO = K - first_class;
    const bool has_act = act != nullptr;
    for (int i = threadIdx.x; i < A; i += blockDim.x) {
        const size_t ai = (size_t)c * A + i;
        // decode_predictions (test.py:114-120)
        decode_segment(ld_map<TWO>(loc, f.loc, ai * 2), ld_map<TWO>(loc, f.loc, ai * 2 + 1),
                       ld_map<TWO>(prop_loc, f.prop_loc, ai * 2), ld_map<TWO>(prop_loc, f.prop_loc, ai * 2 + 1), priors, offsets,
                       fps, seg, ai, i, c, clip_length);
        const auto cf = [&](int k) {             // logit k of the anchor's conf row, pf: of its prop_conf row
            const float z = ld_map<TWO>(conf, f.conf, ai * K + k);
            if constexpr (TWO) return z * f.conf_sign; else return z;
        };
        const auto pf = [&](int k) {
            const float z = ld_map<TWO>(prop_conf, f.prop_conf, ai * K + k);
            if constexpr (TWO) return z * f.conf_sign; else return z;
        };
        float S = 0.f, PS = 0.f, M = 0.f, PM = 0.f;
        if constexpr (SOFTMAX) {
            M = cf(0); PM = pf(0);
            for (int k = 1; k < K; ++k) { M = fmaxf(M, cf(k)); PM = fmaxf(PM, pf(k)); }
            for (int k = 0; k < K; ++k) { S += expf(cf(k) - M); PS += expf(pf(k) - PM); }
        } else if constexpr (EV) {
            for (int k = 0; k < K; ++k) {
                S += otal_ev::alpha(cf(k), evidence);
                PS += otal_ev::alpha(pf(k), evidence);
            }
        } else {
            // Dirichlet mean + uncertainty (BDNet.py:538-561), evidence = exp(clamp(logit, +-10))
            for (int k = 0; k < K; ++k) {
                S += expf(fminf(fmaxf(cf(k), -10.f), 10.f)) + 1.0f;
                PS += expf(fminf(fmaxf(pf(k), -10.f), 10.f)) + 1.0f;
            }
        }
        const float an =
            has_act ? (sigmoidf_(ld_map<TWO>(act, f.act, ai)) + sigmoidf_(ld_map<TWO>(prop_act, f.prop_act, ai))) / 2.0f : 0.f;
        const float ct = sigmoidf_(ld_map<TWO>(center, f.center, ai));
        bool own_unct = false;          // the networks' own uncertainty maps stand in for the one derived from the logits
        if constexpr (TWO) own_unct = f.unct != nullptr;
        if (unct) {
            if (own_unct) unct[ai] = avg2(avg2(f.unct[ai], f.flow_unct[ai]), avg2(f.prop_unct[ai], f.flow_prop_unct[ai]));
            else unct[ai] = SOFTMAX ? 0.f : ((float)K / S + (float)K / PS) / 2.0f;
        }
        if (actn) actn[ai] = an;
        for (int k = first_class; k < K; ++k) {
            float a0, a1;
            if constexpr (SOFTMAX) {
                a0 = expf(cf(k) - M) / S;
                a1 = expf(pf(k) - PM) / PS;
            } else if constexpr (EV) {
                a0 = otal_ev::alpha(cf(k), evidence) / S;
                a1 = otal_ev::alpha(pf(k), evidence) / PS;
            } else {
                a0 = (expf(fminf(fmaxf(cf(k), -10.f), 10.f)) + 1.0f) / S;
                a1 = (expf(fminf(fmaxf(pf(k), -10.f), 10.f)) + 1.0f) / PS;
            }
            const size_t o = ((size_t)c * KO + (k - first_class)) * A + i;
            if (has_act) {
                const float sc = (a0 + a1) / 2.0f * ct * an;
                score[o] = sc;
                flag[o] = (sc > conf_thresh) && (an > 0.5f);       // filtering (test.py:143-147)
            } else {
                const float sc = (a0 + a1) / 2.0f * ct;
                score[o] = sc;
                flag[o] = sc > conf_thresh;
            }
        }
    }
}

struct Best { float v; int i; int n; };   // max undone score, its lowest index, number of undone

__device__ __forceinline__ Best best_merge(Best a, Best b) {
    Best r;
    r.n = a.n + b.n;
    const bool take_b = (b.i >= 0) && (a.i < 0 || b.v > a.v || (b.v == a.v && b.i < a.i));
    r.v = take_b ? b.v : a.v;
    r.i = take_b ? b.i : a.i;
    return r;
}

// One workgroup per (video, class).  Working set: ts, te, sc (float), st (int: 0 dropped, 1 done, 2 undone),
// src (int: row in the clip-major candidate space) for up to `cap` candidates.
// BIG = false: the working set lives in LDS (`cap` = lds_cap rows); a video with more rows than that is left to the
//              BIG launch when one follows (`defer_big`), i.e. this workgroup returns at once.
// BIG = true : the working set lives in a caller-provided global scratch sized for every row of the video (five
//              arrays of total_clips*K*A words; (v,k) owns rows [(clip_start[v]*K + k*clips_v)*A, +clips_v*A)), so a
//              video of any length is handled (the reference's host loop has no limit either, test.py:165-200); only
//              the videos the LDS launch deferred are processed.  All traffic stays inside one workgroup, whose
//              barriers order its own global stores and loads.
template <bool BIG>
__global__ __launch_bounds__(NMS_THREADS) void softnms_classes_kernel(
        const float* __restrict__ seg, const float* __restrict__ score, const float* __restrict__ unct,
        const float* __restrict__ actn, const unsigned char* __restrict__ flag, const int* __restrict__ clip_start,
        float* __restrict__ out, int* __restrict__ counts, int* __restrict__ out_index, int A, int K, int lds_cap,
        float sigma, int top_k, float thr, int out_cols, float* __restrict__ scratch, long long scratch_rows, int defer_big) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ Best red[NMS_THREADS / 64];
    __shared__ int s_n, s_scan[NMS_THREADS / 64 + 1];
    const int v = blockIdx.x / K, k = blockIdx.x % K;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c0 = clip_start[v], c1 = clip_start[v + 1];
    const int total = (c1 - c0) * A;          // rows of this video in clip-major order
    if (BIG ? total <= lds_cap : (defer_big && total > lds_cap)) return;
    const int cap = BIG ? total : lds_cap;
    float* ts; float* te; float* sc; int* st; int* src;
    if constexpr (BIG) {
        const long long o = ((long long)c0 * K + (long long)k * (c1 - c0)) * A;
        ts = scratch + o;
        te = scratch + scratch_rows + o;
        sc = scratch + 2 * scratch_rows + o;
        st = reinterpret_cast<int*>(scratch + 3 * scratch_rows + o);
        src = reinterpret_cast<int*>(scratch + 4 * scratch_rows + o);
    } else {
        ts = reinterpret_cast<float*>(smem);
        te = ts + cap;
        sc = te + cap;
        st = reinterpret_cast<int*>(sc + cap);
        src = st + cap;
    }
    // ---- gather flagged candidates in index order (block scan over chunks of NMS_THREADS rows)
    if (tid == 0) s_n = 0;
    __syncthreads();
    for (int base = 0; base < total; base += NMS_THREADS) {
        const int r = base + tid;
        int f = 0;
        size_t so = 0;
        if (r < total) {
            const int c = c0 + r / A, i = r % A;
            so = ((size_t)c * K + k) * A + i;
            f = flag[so];
        }
        const unsigned long long m = __ballot(f);
        const int before = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) s_scan[wave + 1] = __popcll(m);
        __syncthreads();
        if (tid == 0) {
            s_scan[0] = s_n;
            for (int w = 0; w < NMS_THREADS / 64; ++w) s_scan[w + 1] += s_scan[w];
            s_n = s_scan[NMS_THREADS / 64];
        }
        __syncthreads();
        if (f) {
            const int p = s_scan[wave] + before;
            if (p < cap) {
                const int c = c0 + r / A, i = r % A;
                ts[p] = seg[((size_t)c * A + i) * 2];
                te[p] = seg[((size_t)c * A + i) * 2 + 1];
                sc[p] = score[so];
                st[p] = score[so] >= thr ? 2 : 0;
                src[p] = c * A + i;
            }
        }
        __syncthreads();
    }
    const int n = min(s_n, cap);
    // ---- greedy loop
    int ndone = 0;
    for (;;) {
        Best b = {0.f, -1, 0};
        for (int i = tid; i < n; i += NMS_THREADS)
            if (st[i] == 2) {
                b.n += 1;
                if (b.i < 0 || sc[i] > b.v) { b.v = sc[i]; b.i = i; }     // strided ascending i: first max kept
            }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            Best t;
            t.v = __shfl_down(b.v, o, 64); t.i = __shfl_down(b.i, o, 64); t.n = __shfl_down(b.n, o, 64);
            b = best_merge(b, t);
        }
        if (lane == 0) red[wave] = b;
        __syncthreads();
        b = red[0];
#pragma unroll
        for (int w = 1; w < NMS_THREADS / 64; ++w) b = best_merge(b, red[w]);
        __syncthreads();
        if (b.n <= 1 || ndone >= top_k) break;                 // `undone.sum() > 1 and done.sum() < top_k`
        const int j = b.i;
        const float top_s = ts[j], top_e = te[j];
        const float width = fmaxf(top_e - top_s, 1e-5f);
        if (tid == 0) st[j] = 1;
        ++ndone;
        __syncthreads();
        for (int i = tid; i < n; i += NMS_THREADS)
            if (st[i] == 2) {
                const float a0 = ts[i], a1 = te[i];
                const float inter = fmaxf(fminf(a1, top_e) - fmaxf(a0, top_s), 0.f);
                const float iou = inter / (width + (a1 - a0) - inter);
                const float s = sc[i] * expf(-(iou * iou) / sigma);
                sc[i] = s;
                if (s < thr) st[i] = 0;
            }
        __syncthreads();
    }
    // ---- kept rows, original index order: [start, end, decayed score, unct, actionness]
    if (tid == 0) s_n = 0;
    __syncthreads();
    float* o = out + (size_t)blockIdx.x * top_k * out_cols;
    for (int base = 0; base < n; base += NMS_THREADS) {
        const int i = base + tid;
        const int f = (i < n) && st[i] == 1;
        const unsigned long long m = __ballot(f);
        const int before = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) s_scan[wave + 1] = __popcll(m);
        __syncthreads();
        if (tid == 0) {
            s_scan[0] = s_n;
            for (int w = 0; w < NMS_THREADS / 64; ++w) s_scan[w + 1] += s_scan[w];
            s_n = s_scan[NMS_THREADS / 64];
        }
        __syncthreads();
        if (f) {
            const int p = s_scan[wave] + before;
            float* row = o + (size_t)p * out_cols;
            row[0] = ts[i]; row[1] = te[i]; row[2] = sc[i];
            if (out_cols > 3) row[3] = unct[src[i]];
            if (out_cols > 4) row[4] = actn[src[i]];
            if (out_index) out_index[(size_t)blockIdx.x * top_k + p] = src[i] - c0 * A;
        }
        __syncthreads();
    }
    if (tid == 0) counts[blockIdx.x] = s_n;
}

}  // namespace

namespace {
template <bool TWO>
void launch_decode_clips(const float* loc, const float* prop_loc, const float* priors, const float* conf, const float* prop_conf,
                         const float* center, const float* act, const float* prop_act, const float* offsets, const float* fps,
                         float* seg, float* score, float* unct, float* actn, unsigned char* flag, int nclips, int A, int K,
                         float clip_length, float conf_thresh, int score_fn, int first_class, bool ev, int evidence,
                         const FlowMaps& flow, void* stream) {
    if (score_fn == 1)
        hipLaunchKernelGGL((decode_clips_kernel<true, false, TWO>), dim3(nclips), dim3(128), 0, (hipStream_t)stream, loc, prop_loc,
                           priors, conf, prop_conf, center, act, prop_act, offsets, fps, seg, score, unct, actn, flag, A, K,
                           clip_length, conf_thresh, first_class, 0, flow);
    else if (ev)
        hipLaunchKernelGGL((decode_clips_kernel<false, true, TWO>), dim3(nclips), dim3(128), 0, (hipStream_t)stream, loc, prop_loc,
                           priors, conf, prop_conf, center, act, prop_act, offsets, fps, seg, score, unct, actn, flag, A, K,
                           clip_length, conf_thresh, first_class, evidence, flow);
    else if constexpr (!TWO)        // the two-stream entry takes an evidence kind: it has no use for the exp-only instantiation
        hipLaunchKernelGGL((decode_clips_kernel<false, false, TWO>), dim3(nclips), dim3(128), 0, (hipStream_t)stream, loc,
                           prop_loc, priors, conf, prop_conf, center, act, prop_act, offsets, fps, seg, score, unct, actn, flag, A,
                           K, clip_length, conf_thresh, first_class, 0, flow);
}

// two: the second network of otal_decode_clips_2s (with its conf_sign as the caller gave it), NULL for the single-stream entries
int decode_clips_entry(const float* loc, const float* prop_loc, const float* priors, const float* conf,
                                    const float* prop_conf, const float* center, const float* act,
                                    const float* prop_act, const float* offsets, const float* fps, float* seg,
                                    float* score, float* unct, float* actn, unsigned char* flag, int nclips, int A,
                                    int K, float clip_length, float conf_thresh, int score_fn, int first_class,
                                    bool ev, int evidence, void* stream, const FlowMaps* two = nullptr, int conf_sign = 1) {
    if (!loc || !prop_loc || !priors || !conf || !prop_conf || !center || (!act) != (!prop_act) || !offsets || !fps ||
        !seg || !score || !flag) return OTAL_E_NULL;
    if (two) {
        if (!two->loc || !two->prop_loc || !two->conf || !two->prop_conf || !two->center || (!two->act) != (!act) ||
            (!two->prop_act) != (!act)) return OTAL_E_NULL;
        const int given = !!two->unct + !!two->prop_unct + !!two->flow_unct + !!two->flow_prop_unct;
        if ((given != 0 && given != 4) || (given == 4 && !unct)) return OTAL_E_NULL;
    }
    if (nclips <= 0 || A <= 0 || K <= 0) return OTAL_E_SHAPE;
    if (score_fn < 0 || score_fn > 1 || first_class < 0 || first_class > 1) return OTAL_E_UNSUPPORTED;
    if (K - first_class <= 0) return OTAL_E_SHAPE;
    if (ev && (evidence < 0 || evidence >= otal_ev::EV_KINDS)) return OTAL_E_UNSUPPORTED;
    if (conf_sign != 1 && conf_sign != -1) return OTAL_E_UNSUPPORTED;
    if (two)
        launch_decode_clips<true>(loc, prop_loc, priors, conf, prop_conf, center, act, prop_act, offsets, fps, seg, score, unct,
                                  actn, flag, nclips, A, K, clip_length, conf_thresh, score_fn, first_class, ev, evidence, *two,
                                  stream);
    else
        launch_decode_clips<false>(loc, prop_loc, priors, conf, prop_conf, center, act, prop_act, offsets, fps, seg, score, unct,
                                   actn, flag, nclips, A, K, clip_length, conf_thresh, score_fn, first_class, ev, evidence,
                                   FlowMaps{}, stream);
    return otal_launch_status();
}
}  // namespace

extern "C" int otal_decode_clips_ex(const float* loc, const float* prop_loc, const float* priors, const float* conf,
                                    const float* prop_conf, const float* center, const float* act,
                                    const float* prop_act, const float* offsets, const float* fps, float* seg,
                                    float* score, float* unct, float* actn, unsigned char* flag, int nclips, int A,
                                    int K, float clip_length, float conf_thresh, int score_fn, int first_class,
                                    void* stream) {
    return decode_clips_entry(loc, prop_loc, priors, conf, prop_conf, center, act, prop_act, offsets, fps, seg, score, unct, actn,
                              flag, nclips, A, K, clip_length, conf_thresh, score_fn, first_class, false, 0, stream);
}

// otal_decode_clips_ex with the evidence function of the Dirichlet scores and uncertainty (score_fn 0): 0 exp, 1 relu,
// 2 softplus.  evidence 0 gives bit for bit what otal_decode_clips_ex gives; a kind out of range: OTAL_E_UNSUPPORTED.
extern "C" int otal_decode_clips_ev(const float* loc, const float* prop_loc, const float* priors, const float* conf,
                                    const float* prop_conf, const float* center, const float* act,
                                    const float* prop_act, const float* offsets, const float* fps, float* seg,
                                    float* score, float* unct, float* actn, unsigned char* flag, int nclips, int A,
                                    int K, float clip_length, float conf_thresh, int score_fn, int first_class,
                                    int evidence, void* stream) {
    return decode_clips_entry(loc, prop_loc, priors, conf, prop_conf, center, act, prop_act, offsets, fps, seg, score, unct, actn,
                              flag, nclips, A, K, clip_length, conf_thresh, score_fn, first_class, true, evidence, stream);
}

// otal_decode_clips_ev for two networks: every map value the decode reads is (rgb + flow) / 2 in fp32, taken in registers (ld_map),
// so seg, score, actn and flag are bit for bit otal_decode_clips_ev's on the averaged maps; see include/opental_hip.h.
extern "C" int otal_decode_clips_2s(const float* loc, const float* prop_loc, const float* conf, const float* prop_conf,
                                    const float* center, const float* act, const float* prop_act, const float* flow_loc,
                                    const float* flow_prop_loc, const float* flow_conf, const float* flow_prop_conf,
                                    const float* flow_center, const float* flow_act, const float* flow_prop_act,
                                    const float* unct_in, const float* prop_unct_in, const float* flow_unct_in,
                                    const float* flow_prop_unct_in, const float* priors, const float* offsets,
                                    const float* fps, float* seg, float* score, float* unct, float* actn,
                                    unsigned char* flag, int nclips, int A, int K, float clip_length, float conf_thresh,
                                    int score_fn, int first_class, int evidence, int conf_sign, void* stream) {
    const FlowMaps flow = {flow_loc, flow_prop_loc, flow_conf, flow_prop_conf, flow_center, flow_act, flow_prop_act,
                           unct_in, prop_unct_in, flow_unct_in, flow_prop_unct_in, (float)conf_sign};
    return decode_clips_entry(loc, prop_loc, priors, conf, prop_conf, center, act, prop_act, offsets, fps, seg, score, unct, actn,
                              flag, nclips, A, K, clip_length, conf_thresh, score_fn, first_class, true, evidence, stream, &flow,
                              conf_sign);
}

extern "C" int otal_decode_clips(const float* loc, const float* prop_loc, const float* priors, const float* conf,
                                 const float* prop_conf, const float* center, const float* act,
                                 const float* prop_act, const float* offsets, const float* fps, float* seg,
                                 float* score, float* unct, float* actn, unsigned char* flag, int nclips, int A,
                                 int K, float clip_length, float conf_thresh, void* stream) {
    if (!act || !prop_act || !unct || !actn) return OTAL_E_NULL;       // the OpenTAL head: every map present
    return otal_decode_clips_ex(loc, prop_loc, priors, conf, prop_conf, center, act, prop_act, offsets, fps, seg, score,
                                unct, actn, flag, nclips, A, K, clip_length, conf_thresh, 0, 0, stream);
}

constexpr size_t NMS_LDS_LIMIT = 150 * 1024;      // working set of ~7600 candidates; beyond that the scratch path runs

extern "C" size_t otal_softnms_scratch_bytes(int total_clips, int max_clips, int A, int K) {
    if (total_clips <= 0 || max_clips <= 0 || A <= 0 || K <= 0) return 0;
    if ((size_t)max_clips * A * 20 <= NMS_LDS_LIMIT) return 0;
    return (size_t)total_clips * K * A * 20;
}

extern "C" int otal_softnms_classes_ws(const float* seg, const float* score, const float* unct, const float* actn,
                                       const unsigned char* flag, const int* clip_start, int nvideos, int max_clips,
                                       int A, int K, float sigma, int top_k, float score_threshold, float* out,
                                       int* counts, int* out_index, int out_cols, void* scratch, size_t scratch_bytes,
                                       int total_clips, void* stream) {
    if (nvideos <= 0 || max_clips <= 0 || A <= 0 || K <= 0 || top_k <= 0 || out_cols < 3 || out_cols > 5)
        return OTAL_E_SHAPE;
    // unct is read only for out_cols > 3, actn only for out_cols > 4 (closed-set rows: 3 or 4 columns)
    if (!seg || !score || (out_cols > 3 && !unct) || (out_cols > 4 && !actn) || !flag || !clip_start || !out || !counts)
        return OTAL_E_NULL;
    const size_t need = otal_softnms_scratch_bytes(total_clips, max_clips, A, K);
    const bool big = need != 0;
    if (big && (!scratch || scratch_bytes < need)) return OTAL_E_UNSUPPORTED;   // longest video exceeds LDS: scratch required
    const int lds_cap = big ? (int)(NMS_LDS_LIMIT / 20) : max_clips * A;
    const size_t lds = (size_t)lds_cap * 20;
    if (lds > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(softnms_classes_kernel<false>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    const long long rows = (long long)total_clips * K * A;
    hipLaunchKernelGGL(softnms_classes_kernel<false>, dim3(nvideos * K), dim3(NMS_THREADS), lds, (hipStream_t)stream, seg,
                       score, unct, actn, flag, clip_start, out, counts, out_index, A, K, lds_cap, sigma, top_k, score_threshold,
                       out_cols, (float*)nullptr, 0LL, big ? 1 : 0);
    if (big)
        hipLaunchKernelGGL(softnms_classes_kernel<true>, dim3(nvideos * K), dim3(NMS_THREADS), 0, (hipStream_t)stream, seg,
                           score, unct, actn, flag, clip_start, out, counts, out_index, A, K, lds_cap, sigma, top_k,
                           score_threshold, out_cols, (float*)scratch, rows, 1);
    return otal_launch_status();
}

extern "C" int otal_softnms_classes(const float* seg, const float* score, const float* unct, const float* actn,
                                    const unsigned char* flag, const int* clip_start, int nvideos, int max_clips,
                                    int A, int K, float sigma, int top_k, float score_threshold, float* out,
                                    int* counts, int* out_index, int out_cols, void* stream) {
    // no scratch: every video must fit the LDS working set (OTAL_E_UNSUPPORTED otherwise; use otal_softnms_classes_ws)
    return otal_softnms_classes_ws(seg, score, unct, actn, flag, clip_start, nvideos, max_clips, A, K, sigma, top_k,
                                   score_threshold, out, counts, out_index, out_cols, nullptr, 0,
                                   (size_t)max_clips * A * 20 <= NMS_LDS_LIMIT ? 1 : max_clips, stream);
}
