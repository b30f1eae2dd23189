// opental_amd/csrc/options.h -- the library's named run-time switches.  No HIP types in here: common.h includes it for the
// kernels' translation units, conv_select.h and pool_select.h for the kernel choice, and tests/cpu_options.h serves the defaults
// to their CPU harnesses.
#pragma once

// Named run-time switches: the kernel-selection references the tests flip (otal_set_option).  The table is the only place
// a switch is named with its default; OTAL_OPT("NAME") of a name not in it does not compile.
struct OtalOption { const char* name; int dflt; };
constexpr OtalOption OTAL_OPTIONS[] = {
    {"OTAL_CONV_1A_NOTILE", 0},           {"OTAL_CONV_1A_WGS", 0},      // 0: one workgroup per compute unit
    {"OTAL_CONV_DIRECT_MINTILES", 140},   {"OTAL_CONV_DIRECT_MINTILES512", 512},
    {"OTAL_CONV_DIRECT_XPF2", 3},         {"OTAL_CONV_NO1A", 0},
    {"OTAL_CONV_NO1AW", 0},               {"OTAL_CONV_NO1DTILE", 0},
    {"OTAL_CONV_NO1X1STREAM", 0},         {"OTAL_CONV_NODIRECT", 0},
    {"OTAL_CONV_NOPROJ", 0},              {"OTAL_CONV_NOPROJW", 0},
    {"OTAL_CONV_NOW1D", 0},               {"OTAL_CONV_NOW1X1", 0},
    {"OTAL_CONV_NOWDIRECT", 0},           {"OTAL_LOSS_NOSTAGE", 0},
    {"OTAL_POOL_NO133", 0},               {"OTAL_POOL_NOROWS", 0},
    {"OTAL_W1A_SPLITS", 0},               {"OTAL_WDIRECT_BLOCKS", 0},   // 0: the launcher's own choice
};
constexpr int OTAL_NUM_OPTIONS = sizeof(OTAL_OPTIONS) / sizeof(OTAL_OPTIONS[0]);
constexpr bool otal_streq(const char* a, const char* b) { return *a == *b && (*a == 0 || otal_streq(a + 1, b + 1)); }
constexpr int otal_option_index(const char* name, int i = 0) {
    return i == OTAL_NUM_OPTIONS ? -1 : otal_streq(OTAL_OPTIONS[i].name, name) ? i : otal_option_index(name, i + 1);
}
// The value of switch `index` (core.hip): its first lookup reads the environment variable of the same name (absent: the
// default; present but not a number: 1), later lookups are one load.  Never getenv() on a launch path.
int* otal_option_slot(int index);
#define OTAL_OPT(name) ([]() -> int {                                                                              \
    constexpr int index_ = otal_option_index(name);                                                              \
    static_assert(index_ >= 0, "unknown option " name " (options.h: OTAL_OPTIONS)");                               \
    static int* const slot_ = otal_option_slot(index_);                                                          \
    return *slot_;                                                                                               \
}())
