// tests/cpu_options.h -- the library's run-time switches for the CPU harnesses (cpu_conv_select.cpp, cpu_pool_select.cpp): they
// answer with their table defaults (options.h), whatever the environment says, unless cpu_set_option() changes one.
#pragma once
#include <cstring>
#include "options.h"

static int g_options[OTAL_NUM_OPTIONS];
static bool g_options_set = false;

int* otal_option_slot(int index) {
    if (!g_options_set) {
        for (int i = 0; i < OTAL_NUM_OPTIONS; ++i) g_options[i] = OTAL_OPTIONS[i].dflt;
        g_options_set = true;
    }
    return &g_options[index];
}

extern "C" int cpu_set_option(const char* name, int value) {
    for (int i = 0; i < OTAL_NUM_OPTIONS; ++i)
        if (!strcmp(OTAL_OPTIONS[i].name, name)) { *otal_option_slot(i) = value; return 0; }
    return -1;
}
