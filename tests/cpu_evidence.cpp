// tests/cpu_evidence.cpp -- plain-C++ harness of opental_amd/csrc/evidence.h for tests/test_evidence_cpu.py: the functions the
// kernels call, evaluated on arrays.
#include <stddef.h>
#include "evidence.h"

extern "C" {

void cpu_ev_alpha(const float* z, int n, int evidence, float* out) {
    for (int i = 0; i < n; ++i) out[i] = otal_ev::alpha(z[i], evidence);
}

void cpu_ev_dalpha(const float* z, int n, int evidence, float* out) {
    for (int i = 0; i < n; ++i) out[i] = otal_ev::dalpha(z[i], evidence);
}

void cpu_ev_digamma(const float* x, int n, float* out) {
    for (int i = 0; i < n; ++i) out[i] = otal_ev::digammaf_(x[i]);
}

void cpu_ev_trigamma(const float* x, int n, float* out) {
    for (int i = 0; i < n; ++i) out[i] = otal_ev::trigammaf_(x[i]);
}

// rows (n, C) of logits against labels y (n): per (n) and d per / d alpha (n, C)
void cpu_ev_cls_rows(const float* z, const int* y, int n, int C, int evidence, int loss_type, float* per, float* dper) {
    for (int i = 0; i < n; ++i) {
        const otal_ev::ClsRow r = otal_ev::cls_row(z + (size_t)i * C, C, y[i], evidence, loss_type);
        per[i] = r.per;
        for (int k = 0; k < C; ++k)
            dper[(size_t)i * C + k] = otal_ev::cls_dalpha(r, otal_ev::alpha(z[(size_t)i * C + k], evidence), k == y[i], loss_type);
    }
}

}  // extern "C"
