// opental_amd/csrc/core.hip -- ABI version + error strings for libopental_hip.so.
#include "common.h"

extern "C" int otal_abi_version(void) { return OTAL_ABI_VERSION; }

extern "C" const char* otal_error_string(int code) {
    switch (code) {
        case 0: return "success";
        case OTAL_E_NULL: return "null pointer argument";
        case OTAL_E_SHAPE: return "non-positive or inconsistent size";
        case OTAL_E_ODD_C: return "BoundaryMaxPooling needs an even channel count";
        case OTAL_E_BATCH: return "segments batch differs from feature batch";
        case OTAL_E_DTYPE: return "unsupported dtype code";
        case OTAL_E_LEVELS: return "bad level table";
        case OTAL_E_UNSUPPORTED: return "configuration not supported by this build";
        default: break;
    }
    if (code > 0) return hipGetErrorString((hipError_t)code);
    return "unknown error";
}

// ---- run-time switches (options.h: OTAL_OPTIONS) --------------------------------------------------------------------
// A switch takes its initial value from the environment variable of the same name, read ONCE at its first lookup: the
// launch path never calls getenv (it used to, ~10 times per convolution launch).  otal_set_option changes a switch at run
// time; a name that is not in the table is refused.
#include <cstdlib>
#include <cstring>
#include <mutex>
namespace {
int g_option_value[OTAL_NUM_OPTIONS];
bool g_option_set[OTAL_NUM_OPTIONS];       // value holds (read from the environment, or set by otal_set_option)
std::mutex g_options_mutex;
int option_index(const char* name) {
    for (int i = 0; i < OTAL_NUM_OPTIONS; ++i)
        if (!strcmp(OTAL_OPTIONS[i].name, name)) return i;
    return -1;
}
}  // namespace

int* otal_option_slot(int index) {
    std::lock_guard<std::mutex> lock(g_options_mutex);
    if (!g_option_set[index]) {
        int v = OTAL_OPTIONS[index].dflt;
        if (const char* e = getenv(OTAL_OPTIONS[index].name)) {      // present: its number; present but not a number (or empty): 1
            v = atoi(e);
            if (v == 0 && e[0] != '0') v = 1;
        }
        g_option_value[index] = v;
        g_option_set[index] = true;
    }
    return &g_option_value[index];
}

extern "C" int otal_set_option(const char* name, int value) {
    if (!name) return OTAL_E_NULL;
    const int i = option_index(name);
    if (i < 0) return OTAL_E_UNSUPPORTED;
    std::lock_guard<std::mutex> lock(g_options_mutex);
    g_option_value[i] = value;
    g_option_set[i] = true;
    return 0;
}

extern "C" int otal_get_option(const char* name, int dflt) {
    if (!name) return dflt;
    const int i = option_index(name);
    return i < 0 ? dflt : *otal_option_slot(i);
}

// ---- the kernel that served this thread's most recent max-pool / GroupNorm / glue call (common.h: otal_layer_launched)
thread_local const char* g_layer_kernel = "";
extern "C" const char* otal_layer_last_kernel(void) { return g_layer_kernel; }

// ---- stream fork / join ---------------------------------------------------------------------------------------------
// A ring of events: hipStreamWaitEvent takes the event's state at the time of the call, so an event may be recorded again
// once its wait has been issued.
extern "C" int otal_stream_wait(void* waiter, void* signaler) {
    constexpr int RING = 64;
    static hipEvent_t ring[RING];
    static int made = 0, next = 0;
    static std::mutex m;
    if (waiter == signaler) return 0;
    std::lock_guard<std::mutex> lock(m);
    if (made < RING && next == made) {
        if (hipError_t e = hipEventCreateWithFlags(&ring[made], hipEventDisableTiming)) return (int)e;
        ++made;
    }
    hipEvent_t ev = ring[next];
    next = (next + 1) % RING;
    if (hipError_t e = hipEventRecord(ev, (hipStream_t)signaler)) return (int)e;
    if (hipError_t e = hipStreamWaitEvent((hipStream_t)waiter, ev, 0)) return (int)e;
    return 0;
}
