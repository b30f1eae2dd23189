// tests/cpu_pool_select.cpp -- CPU harness: the kernel choice of the max-pools (opental_amd/csrc/pool_select.h), compiled with
// g++ by tests/pool_select_harness.py.  The run-time switches: tests/cpu_options.h.
#include "pool_select.h"
#include "cpu_options.h"

extern "C" int cpu_pool_kernel_count(void) { return PK_COUNT; }
extern "C" const char* cpu_pool_kernel_name(int kernel) { return pool_kernel_name(kernel); }
extern "C" int64_t cpu_pool_lds_budget(void) { return (int64_t)POOL_LDS_BUDGET; }

// flags: fwd {io, nonneg, has_signbits}, bwd {io, accumulate, has_mask, has_scale, has_signbits} (oracle.layer_ref.FIELDS);
// addr: the addresses (or their residues mod 16) in the order of oracle.layer_ref.ADDRS (fwd x, y, argtap, signbits, -;
// bwd dy, dx, argtap, signbits, mask).  out: rc, kernel, grid x, grid y, LDS bytes, planes per block, tlo_max, vec.
extern "C" void cpu_pool_choose(int dir, const int* d, const int64_t* s, const int* flags, const int64_t* addr, int64_t* out) {
    PoolQuery q = {};
    q.dir = dir;
    q.geom_rc = fill(q.g, d, s);
    if (dir == POOL_FWD) {
        q.nonneg = flags[1]; q.has_signbits = flags[2];
        q.io = flags[0] | (q.nonneg ? 4 : 0);
        q.x = (uintptr_t)addr[0]; q.y = (uintptr_t)addr[1];
    } else {
        q.io = flags[0]; q.accumulate = flags[1]; q.has_mask = flags[2]; q.has_scale = flags[3]; q.has_signbits = flags[4];
        q.y = (uintptr_t)addr[0]; q.x = (uintptr_t)addr[1];
        q.mask = q.has_mask ? (uintptr_t)addr[4] : 0;
    }
    q.argtap = (uintptr_t)addr[2];
    q.signbits = q.has_signbits ? (uintptr_t)addr[3] : 0;
    const PoolChoice c = pool_choose(q);
    const int64_t res[8] = {c.rc, c.kernel, c.gx, c.gy, (int64_t)c.lds, c.planes, c.tlo_max, c.vec};
    for (int i = 0; i < 8; ++i) out[i] = res[i];
}
