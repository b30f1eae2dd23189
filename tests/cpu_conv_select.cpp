// tests/cpu_conv_select.cpp -- CPU harness: the kernel choice of the convolution library (opental_amd/csrc/conv_select.h),
// compiled with g++ by tests/test_conv_select_cpu.py.  The run-time switches: tests/cpu_options.h.
#include "conv_select.h"
#include "cpu_options.h"

static void fill(ConvGeom& g, const int* d, const int64_t* s) {
    g.B = d[0]; g.Cin = d[1]; g.Cout = d[2]; g.Ti = d[3]; g.Hi = d[4]; g.Wi = d[5];
    g.To = d[6]; g.Ho = d[7]; g.Wo = d[8]; g.kt = d[9]; g.kh = d[10]; g.kw = d[11];
    g.st = d[12]; g.sh = d[13]; g.sw = d[14]; g.pt = d[15]; g.ph = d[16]; g.pw = d[17];
    g.nlev = d[18];
    for (int i = 0; i <= OTAL_CONV_MAX_LEVELS; ++i) g.lev[i] = d[19 + i];
    g.x_bs = s[0]; g.x_cs = s[1]; g.y_bs = s[2]; g.y_cs = s[3];
}

extern "C" const char* cpu_kernel_name(int kernel) { return conv_kernel_name(kernel); }

// addr: the addresses (or their residues mod 16) of x, w, dy, out, mask.  out[0] = steps, out[1] = prologue layout, then per
// step {kernel, vector width, 1 when OTAL_E_UNSUPPORTED moves on}.
extern "C" void cpu_conv_plan(const int* d, const int64_t* s, int mode, int precision, int accumulate, int has_mask,
                              const int64_t* addr, int* out) {
    ConvQuery q = {};
    fill(q.g, d, s);
    q.mode = mode; q.precision = precision; q.accumulate = accumulate; q.has_mask = has_mask;
    q.x = (uintptr_t)addr[0]; q.w = (uintptr_t)addr[1]; q.dy = (uintptr_t)addr[2]; q.out = (uintptr_t)addr[3]; q.mask = (uintptr_t)addr[4];
    const ConvPlan p = conv_plan(q);
    out[0] = p.n;
    out[1] = p.prologue;
    for (int i = 0; i < p.n; ++i) {
        out[2 + 3 * i] = p.step[i].kernel;
        out[3 + 3 * i] = p.step[i].cw;
        out[4 + 3 * i] = p.step[i].next ? 1 : 0;
    }
}

extern "C" int64_t cpu_prologue_bytes(const int* d, const int64_t* s, int mode, int precision) {
    ConvGeom g;
    fill(g, d, s);
    return (int64_t)conv_prologue_bytes(g, mode, precision & 1);
}

extern "C" int cpu_half_storage(const int* d, const int64_t* s, int mode, int precision) {
    ConvGeom g;
    fill(g, d, s);
    return conv_half_storage(g, mode, precision);
}
