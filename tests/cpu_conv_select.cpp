// tests/cpu_conv_select.cpp -- CPU harness: the kernel choice, launch shapes and workspace query of the convolution library
// (opental_amd/csrc/conv_select.h), compiled with g++ by tests/test_conv_select_cpu.py.  The run-time switches: tests/cpu_options.h.
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

// One step of the call's plan at a workspace of ws_bytes (conv_launch_shape).  out: 0 refuse, 1 front bytes, 2 slab bytes,
// 3 splits, 4 per_split, 5..7 grid, 8 tm, 9 tn, 10 kernel, 11 the step moves on when it refuses;
// returns the plan's length.
extern "C" int cpu_launch_shape(const int* d, const int64_t* s, int mode, int precision, int accumulate, int has_mask,
                                const int64_t* addr, int step, uint64_t ws_bytes, int64_t* out) {
    ConvQuery q = {};
    fill(q.g, d, s);
    q.mode = mode; q.precision = precision; q.accumulate = accumulate; q.has_mask = has_mask;
    q.x = (uintptr_t)addr[0]; q.w = (uintptr_t)addr[1]; q.dy = (uintptr_t)addr[2]; q.out = (uintptr_t)addr[3]; q.mask = (uintptr_t)addr[4];
    const ConvPlan p = conv_plan(q);
    if (step >= p.n) return p.n;
    const ConvLaunchShape sh = conv_launch_shape(q, p.step[step], out, (size_t)ws_bytes);
    const int64_t v[12] = {sh.refuse, (int64_t)sh.front_bytes, (int64_t)sh.slab_bytes, sh.splits, sh.per_split, sh.grid[0], sh.grid[1],
                           sh.grid[2], sh.tm, sh.tn, p.step[step].kernel, p.step[step].next};
    for (int i = 0; i < 12; ++i) out[i] = v[i];
    return p.n;
}

extern "C" uint64_t cpu_workspace_bytes(const int* d, const int64_t* s, int mode) {
    ConvGeom g;
    fill(g, d, s);
    return conv_workspace_bytes(g, mode);
}

// fit_splits with a workspace of ws_bytes at a null or a non-null address.  out: splits, per_split, slab bytes
extern "C" void cpu_fit_splits(int want, int units, int round, uint64_t slab1, int null_ws, uint64_t ws_bytes, int64_t* out) {
    ConvLaunchShape f = {};
    f.N = (int)(slab1 / sizeof(float));         // one row of N floats per slab
    fit_splits(f, 1, want, units, round, null_ws ? nullptr : out, (size_t)ws_bytes);
    out[0] = f.splits; out[1] = f.per_split; out[2] = (int64_t)f.slab_bytes;
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

#ifdef CPU_CONV_SELECT_WALK
// Stand-alone program (built with -fsanitize=address,undefined by tests/test_conv_select_cpu.py): every call of the file --
// 41 numbers a line: geometry, strides, mode, precision, accumulate, has_mask, addresses -- as recorded and on fp32 operands,
// every step of its plan, at no workspace, one byte, the query's size and 192 MiB.
#include <cstdio>
int main(int argc, char** argv) {
    FILE* f = argc > 1 ? fopen(argv[1], "r") : nullptr;
    if (!f) return 2;
    long long v[41], walked = 0, sum = 0;
    for (;;) {
        int n = 0;
        while (n < 41 && fscanf(f, "%lld", &v[n]) == 1) ++n;
        if (n < 41) break;
        int d[28];
        int64_t s[4];
        for (int i = 0; i < 28; ++i) d[i] = (int)v[i];
        for (int i = 0; i < 4; ++i) s[i] = v[28 + i];
        ConvQuery q = {};
        fill(q.g, d, s);
        q.mode = (int)v[32]; q.accumulate = (int)v[34]; q.has_mask = (int)v[35];
        q.x = (uintptr_t)v[36]; q.w = (uintptr_t)v[37]; q.dy = (uintptr_t)v[38]; q.out = (uintptr_t)v[39]; q.mask = (uintptr_t)v[40];
        const size_t sizes[4] = {0, 1, conv_workspace_bytes(q.g, q.mode), (size_t)192 << 20};
        const int precisions[2] = {(int)v[33], q.mode == MODE_DGRAD ? 2 : 0};
        for (const int precision : precisions) {
            q.precision = precision;
            const ConvPlan p = conv_plan(q);
            for (int j = 0; j < p.n; ++j)
                for (const size_t ws_bytes : sizes) {
                    const ConvLaunchShape sh = conv_launch_shape(q, p.step[j], &q, ws_bytes);
                    if (!sh.refuse && sh.front_bytes + sh.slab_bytes > ws_bytes) return 3;      // the cut stays inside what was offered
                    sum += sh.splits + sh.grid[0] + sh.grid[1] + sh.grid[2];
                    ++walked;
                }
        }
    }
    fclose(f);
    printf("%lld shapes, checksum %lld\n", walked, sum);
    return walked > 0 ? 0 : 4;
}
#endif
