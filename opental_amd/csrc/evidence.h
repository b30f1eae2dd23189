// opental_amd/csrc/evidence.h -- the arithmetic of evidential deep learning in one place: the three evidence functions of the
// reference's DirichletLayer / EvidenceLoss (BDNet.py:538-556, cls_loss.py:182-190) with torch's backward conventions, fp32
// digamma / trigamma for arguments >= 1, and the per-row classification term of the three loss types (cls_loss.py:193-285)
// with its derivative with respect to alpha_k.  Shared by loss.hip, heads.hip, infer.hip and anchorstats.hip (the kernels
// that take an evidence kind call these functions and nothing else for evidence and loss arithmetic) and by a plain-C++ CPU
// harness (tests/cpu_evidence.cpp) that compares them against float64.  No HIP types in here.  The ActivityNet loss kernel,
// whose anchors have four lanes each, evaluates a row through the lane-share functions at the end of this file
// (tests/cpu_evidence_lanes.cpp).
//
//   evidence   0 exp       e = exp(clamp(z, -10, 10));   de/dz = exp(z) for -10 <= z <= 10 (inclusive, clamp's backward), else 0
//              1 relu      e = max(z, 0);                de/dz = 1 for z > 0, else 0 (0 at z == 0)
//              2 softplus  e = z for z > 20, else log1p(exp(z));   de/dz = 1 for z > 20, else exp(z) / (exp(z) + 1)
//   loss_type  0 log       log S - log alpha_y
//              1 digamma   psi(S) - psi(alpha_y)
//              2 mse       sum_k (y_k - alpha_k / S)^2 + sum_k alpha_k (S - alpha_k) / (S^2 (S + 1))
// alpha = e + 1 >= 1 and S = sum_k alpha_k >= C always; with exp evidence S reaches 16 (e^10 + 1) = 3.5e5.
#pragma once
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define OTAL_EV_FN __host__ __device__ inline
#else
#define OTAL_EV_FN inline
#endif

namespace otal_ev {

enum { EV_EXP = 0, EV_RELU = 1, EV_SOFTPLUS = 2, EV_KINDS = 3 };
enum { LOSS_LOG = 0, LOSS_DIGAMMA = 1, LOSS_MSE = 2, LOSS_TYPES = 3 };

// alpha = e(z) + 1
OTAL_EV_FN float alpha(float z, int evidence) {
    if (evidence == EV_RELU) return fmaxf(z, 0.f) + 1.f;
    if (evidence == EV_SOFTPLUS) return (z > 20.f ? z : log1pf(expf(z))) + 1.f;
    return expf(fminf(fmaxf(z, -10.f), 10.f)) + 1.f;
}

// d alpha / d z
OTAL_EV_FN float dalpha(float z, int evidence) {
    if (evidence == EV_RELU) return z > 0.f ? 1.f : 0.f;
    if (evidence == EV_SOFTPLUS) {
        if (z > 20.f) return 1.f;
        const float e = expf(z);
        return e / (e + 1.f);
    }
    return (z >= -10.f && z <= 10.f) ? expf(z) : 0.f;
}

// psi(x), x >= 1: the recurrence psi(x) = psi(x + 1) - 1 / x up to x >= 6 (the 1 / x are summed first and subtracted once), then
// log x - 1/(2x) - 1/(12 x^2) + 1/(120 x^4) - 1/(252 x^6); the first term left out is 1/(240 x^8) < 2.5e-9 there
OTAL_EV_FN float digammaf_(float x) {
    float back = 0.f;
    while (x < 6.f) { back += 1.f / x; x += 1.f; }
    const float r = 1.f / x, r2 = r * r;
    const float tail = r2 * (1.f / 12.f - r2 * (1.f / 120.f - r2 * (1.f / 252.f)));
    return ((logf(x) - 0.5f * r) - tail) - back;
}

// psi'(x), x >= 1: psi'(x) = psi'(x + 1) + 1 / x^2 up to x >= 6, then 1/x + 1/(2 x^2) + 1/(6 x^3) - 1/(30 x^5) + 1/(42 x^7);
// the first term left out is 1/(30 x^9) < 3.4e-9 there
OTAL_EV_FN float trigammaf_(float x) {
    float back = 0.f;
    while (x < 6.f) { back += 1.f / (x * x); x += 1.f; }
    const float r = 1.f / x, r2 = r * r;
    const float series = r + r2 * (0.5f + r * (1.f / 6.f - r2 * (1.f / 30.f - r2 * (1.f / 42.f))));
    return series + back;
}

// One row of logits against the class y: S, alpha_y, the classification term `per` and what its derivative needs,
//   d per / d alpha_k = dS + c1 * alpha_k - [k == y] dY          (c1 != 0 for mse only),
// plus the row's |z|_1 and its first largest alpha (the re-weighting rules of the loss read them).  y outside [0, C) gives
// alpha_y = 1 (a row that is not classified; only S is used of it).
struct ClsRow { float S, ay, per, dS, dY, c1, l1, amax; int kmax; };

OTAL_EV_FN float cls_dalpha(const ClsRow& r, float alpha_k, bool is_y, int loss_type) {
    if (loss_type == LOSS_MSE) return (r.dS + r.c1 * alpha_k) - (is_y ? r.dY : 0.f);
    return r.dS - (is_y ? r.dY : 0.f);
}

OTAL_EV_FN ClsRow cls_row(const float* z, int C, int y, int evidence, int loss_type) {
    ClsRow r;
    float S = 0.f, l1 = 0.f, ay = 1.f, amax = 0.f;
    int kmax = 0;
    for (int k = 0; k < C; ++k) {
        const float a = alpha(z[k], evidence);
        S += a;
        l1 += fabsf(z[k]);
        if (k == y) ay = a;
        if (a > amax) { amax = a; kmax = k; }
    }
    r.S = S; r.ay = ay; r.l1 = l1; r.amax = amax; r.kmax = kmax; r.c1 = 0.f;
    if (loss_type == LOSS_LOG) {
        r.per = logf(S) - logf(ay);
        r.dS = 1.f / S; r.dY = 1.f / ay;
    } else if (loss_type == LOSS_DIGAMMA) {
        r.per = digammaf_(S) - digammaf_(ay);
        r.dS = trigammaf_(S); r.dY = trigammaf_(ay);
    } else {
        // err = sum_k (y_k - p_k)^2 with p = alpha / S, var = sum_k alpha_k (S - alpha_k) / (S^2 (S + 1)) = (1 - sum p^2) / (S + 1):
        //   d err / d alpha_j = (2 / S) (p_j - y_j - T),  T = sum_k (p_k - y_k) p_k = sum p^2 - p_y
        //   d var / d alpha_j = 2 (S - alpha_j) / (S^2 (S + 1)) - (1 - sum p^2) (3 S + 2) / (S (S + 1)^2)
        float err = 0.f, var = 0.f, p2 = 0.f;
        const float den = S * S * (S + 1.f);
        for (int k = 0; k < C; ++k) {
            const float a = alpha(z[k], evidence), p = a / S, d = (k == y ? 1.f : 0.f) - p;
            err += d * d;
            var += a * (S - a) / den;
            p2 += p * p;
        }
        r.per = err + var;
        const float T = p2 - ay / S;
        r.c1 = 2.f / (S * (S + 1.f));                                   // 2 / S^2 - 2 / (S^2 (S + 1))
        r.dS = (2.f / (S * (S + 1.f)) - 2.f * T / S) - (1.f - p2) * (3.f * S + 2.f) / (S * (S + 1.f) * (S + 1.f));
        r.dY = 2.f / S;
    }
    return r;
}

// ---- one row evaluated in lane shares: its classes dealt out as c = sub, sub + nsub, ... to nsub cooperating lanes (the
// ActivityNet loss kernel: four lanes per anchor).  Each lane makes a partial pass over its classes, the caller combines the
// partials (S, l1, ay: sums -- a lane that does not own class y leaves ay 0, and alpha >= 1, so a combined 0 means "row not
// classified"; amax: maximum), and row_finish gives cls_row's fields.  mse needs a second partial pass once the combined S is
// known (err, var, sum p^2: sums).  With nsub = 1 the operations and their order are cls_row's: the same bits.  kmax is not
// tracked across lanes (-1).
struct RowPart { float S, l1, ay, amax; };
struct MsePart { float err, var, p2; };

OTAL_EV_FN RowPart row_part(const float* z, int C, int y, int evidence, int sub, int nsub) {
    RowPart p;
    p.S = 0.f; p.l1 = 0.f; p.ay = 0.f; p.amax = 0.f;
    for (int k = sub; k < C; k += nsub) {
        const float a = alpha(z[k], evidence);
        p.S += a;
        p.l1 += fabsf(z[k]);
        if (k == y) p.ay = a;
        if (a > p.amax) p.amax = a;
    }
    return p;
}

// S: the row's combined sum of alpha
OTAL_EV_FN MsePart mse_part(const float* z, int C, int y, int evidence, float S, int sub, int nsub) {
    MsePart m;
    m.err = 0.f; m.var = 0.f; m.p2 = 0.f;
    const float den = S * S * (S + 1.f);
    for (int k = sub; k < C; k += nsub) {
        const float a = alpha(z[k], evidence), p = a / S, d = (k == y ? 1.f : 0.f) - p;
        m.err += d * d;
        m.var += a * (S - a) / den;
        m.p2 += p * p;
    }
    return m;
}

// t, m: the combined partials (m is read for mse only)
OTAL_EV_FN ClsRow row_finish(const RowPart& t, const MsePart& m, int loss_type) {
    ClsRow r;
    const float S = t.S, ay = t.ay > 0.f ? t.ay : 1.f;
    r.S = S; r.ay = ay; r.l1 = t.l1; r.amax = t.amax; r.kmax = -1; r.c1 = 0.f;
    if (loss_type == LOSS_LOG) {
        r.per = logf(S) - logf(ay);
        r.dS = 1.f / S; r.dY = 1.f / ay;
    } else if (loss_type == LOSS_DIGAMMA) {
        r.per = digammaf_(S) - digammaf_(ay);
        r.dS = trigammaf_(S); r.dY = trigammaf_(ay);
    } else {                            // the formulas of cls_row
        r.per = m.err + m.var;
        const float T = m.p2 - ay / S;
        r.c1 = 2.f / (S * (S + 1.f));
        r.dS = (2.f / (S * (S + 1.f)) - 2.f * T / S) - (1.f - m.p2) * (3.f * S + 2.f) / (S * (S + 1.f) * (S + 1.f));
        r.dY = 2.f / S;
    }
    return r;
}

}  // namespace otal_ev
