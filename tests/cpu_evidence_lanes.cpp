// tests/cpu_evidence_lanes.cpp -- plain-C++ harness of the lane-share row functions of opental_amd/csrc/evidence.h (row_part,
// mse_part, row_finish) for tests/test_anet_evidence_cpu.py: a row dealt out to nsub lanes, the partials combined with a
// plain loop in lane order (the kernel combines with two shuffles), next to the serial cls_row.
#include <stddef.h>
#include "evidence.h"

namespace {
otal_ev::ClsRow split_row(const float* z, int C, int y, int evidence, int loss_type, int nsub) {
    otal_ev::RowPart t = otal_ev::row_part(z, C, y, evidence, 0, nsub);
    for (int s = 1; s < nsub; ++s) {
        const otal_ev::RowPart p = otal_ev::row_part(z, C, y, evidence, s, nsub);
        t.S += p.S; t.l1 += p.l1; t.ay += p.ay;
        if (p.amax > t.amax) t.amax = p.amax;
    }
    otal_ev::MsePart m;
    m.err = m.var = m.p2 = 0.f;
    if (loss_type == otal_ev::LOSS_MSE) {
        m = otal_ev::mse_part(z, C, y, evidence, t.S, 0, nsub);
        for (int s = 1; s < nsub; ++s) {
            const otal_ev::MsePart p = otal_ev::mse_part(z, C, y, evidence, t.S, s, nsub);
            m.err += p.err; m.var += p.var; m.p2 += p.p2;
        }
    }
    return otal_ev::row_finish(t, m, loss_type);
}

void put(const otal_ev::ClsRow& r, float* f) {
    f[0] = r.per; f[1] = r.dS; f[2] = r.dY; f[3] = r.c1; f[4] = r.S; f[5] = r.ay; f[6] = r.l1; f[7] = r.amax;
}
}  // namespace

extern "C" {

// rows (n, C) against labels y (n), each row split over nsub lanes: fields (n, 8) = per, dS, dY, c1, S, ay, l1, amax and
// d per / d alpha (n, C) through cls_dalpha
void cpu_ev_lane_rows(const float* z, const int* y, int n, int C, int evidence, int loss_type, int nsub, float* fields, float* dper) {
    for (int i = 0; i < n; ++i) {
        const float* zi = z + (size_t)i * C;
        const otal_ev::ClsRow r = split_row(zi, C, y[i], evidence, loss_type, nsub);
        put(r, fields + 8 * (size_t)i);
        for (int k = 0; k < C; ++k)
            dper[(size_t)i * C + k] = otal_ev::cls_dalpha(r, otal_ev::alpha(zi[k], evidence), k == y[i], loss_type);
    }
}

// the serial cls_row on the same rows: fields (n, 8)
void cpu_ev_serial_rows(const float* z, const int* y, int n, int C, int evidence, int loss_type, float* fields) {
    for (int i = 0; i < n; ++i) put(otal_ev::cls_row(z + (size_t)i * C, C, y[i], evidence, loss_type), fields + 8 * (size_t)i);
}

}  // extern "C"
