"""The CPU harness of the max-pool kernel choice (tests/cpu_pool_select.cpp over opental_amd/csrc/pool_select.h), for
tests/test_pool_select_cpu.py and tests/test_layer_calls_gpu.py."""
import ctypes
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
NGEOM = 17      # oracle.layer_ref.GEOM, then the four strides, then the family's flags


def build(out_dir):
    out = os.path.join(str(out_dir), "libcpupoolselect.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-std=c++17",
                           "-I" + os.path.join(REPO, "opental_amd", "csrc"),
                           os.path.join(HERE, "cpu_pool_select.cpp"), "-o", out])
    H = ctypes.CDLL(out)
    H.cpu_pool_kernel_name.restype = ctypes.c_char_p
    H.cpu_pool_lds_budget.restype = ctypes.c_int64
    return H


def kernel_names(H):
    return [H.cpu_pool_kernel_name(k).decode() for k in range(H.cpu_pool_kernel_count())]


def choose(H, family, ints, addr, switches=()):
    """pool_choose() for one call: ints in the layout of oracle.layer_ref.FIELDS[family] as passed, addr the five addresses
    (or residues) in the order of ADDRS[family]; the named switches are on for this question only.  -> dict(rc, kernel (name,
    "" when refused), gx, gy, lds, planes, tlo_max, vec)."""
    nflags = {"pool_fwd": 3, "pool_bwd": 5}[family]
    ints = [int(v) for v in ints]
    ga = (ctypes.c_int * NGEOM)(*ints[:NGEOM])
    sa = (ctypes.c_int64 * 4)(*ints[NGEOM:NGEOM + 4])
    fa = (ctypes.c_int * nflags)(*ints[NGEOM + 4:NGEOM + 4 + nflags])
    ad = (ctypes.c_int64 * 5)(*[int(v) for v in addr])
    out = (ctypes.c_int64 * 8)()
    for n in switches:
        assert H.cpu_set_option(n.encode(), 1) == 0, n
    try:
        H.cpu_pool_choose(0 if family == "pool_fwd" else 1, ga, sa, fa, ad, out)
    finally:
        for n in switches:
            assert H.cpu_set_option(n.encode(), 0) == 0         # both pool switches default to 0 (options.h)
    c = dict(zip(("rc", "kernel", "gx", "gy", "lds", "planes", "tlo_max", "vec"), [int(v) for v in out]))
    c["kernel"] = H.cpu_pool_kernel_name(c["kernel"]).decode() if c["rc"] == 0 else ""
    return c
