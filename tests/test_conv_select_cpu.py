"""CPU: which kernel each convolution of the model gets.  The selection (opental_amd/csrc/conv_select.h) is compiled with g++
through tests/cpu_conv_select.cpp and asked about every otal_conv_fwd / _dgrad / _wgrad call of an eager THUMOS14 training
step at b = 8 and b = 1, an ActivityNet step at b = 2 and an inference batch (tests/golden/conv_calls.npz, written by
tools/record_conv_calls.py).  The harness serves the options' table defaults, so this pins the product's choice whatever
the environment sets (conftest.py lowers OTAL_CONV_DIRECT_MINTILES for the GPU tests)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cpuselect") / "libcpuselect.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-std=c++17",
                           "-I" + os.path.join(REPO, "opental_amd", "csrc"),
                           os.path.join(HERE, "cpu_conv_select.cpp"), "-o", out])
    L = ctypes.CDLL(out)
    L.cpu_kernel_name.restype = ctypes.c_char_p
    L.cpu_prologue_bytes.restype = ctypes.c_int64
    return L


@pytest.fixture(scope="module")
def calls(golden_dir):
    return np.load(os.path.join(golden_dir, "conv_calls.npz"))


def plan(lib, z, i):
    """(chain, prologue layout) of call i: kernel names joined by '>', '*' after those that move on when they refuse."""
    ga = (ctypes.c_int * z["geom"].shape[1])(*[int(v) for v in z["geom"][i]])
    sa = (ctypes.c_int64 * 4)(*[int(v) for v in z["strides"][i]])
    ad = (ctypes.c_int64 * 5)(*[int(v) for v in z["addr16"][i]])
    out = (ctypes.c_int * 32)()
    lib.cpu_conv_plan(ga, sa, int(z["mode"][i]), int(z["precision"][i]), int(z["accumulate"][i]), int(z["has_mask"][i]), ad, out)
    steps = []
    for j in range(out[0]):
        k, cw, nxt = out[2 + 3 * j], out[3 + 3 * j], out[4 + 3 * j]
        name = lib.cpu_kernel_name(k).decode()
        steps.append(name + (str(cw) if name == "vector" else "") + ("*" if nxt else ""))
    return ">".join(steps), int(out[1])


def test_every_recorded_call_gets_its_kernels(lib, calls):
    z = calls
    assert len(z["mode"]) > 100 and set(z["source"]) == {"thumos_b8", "thumos_b1", "anet_b2", "inference"}
    bad = []
    for i in range(len(z["mode"])):
        chain, layout = plan(lib, z, i)
        ga = (ctypes.c_int * z["geom"].shape[1])(*[int(v) for v in z["geom"][i]])
        sa = (ctypes.c_int64 * 4)(*[int(v) for v in z["strides"][i]])
        mode, prec = int(z["mode"][i]), int(z["precision"][i])
        got = (chain.split(">")[0], chain, layout, int(lib.cpu_prologue_bytes(ga, sa, mode, prec)),
               int(lib.cpu_half_storage(ga, sa, mode, prec)), int(lib.cpu_half_storage(ga, sa, mode, prec | 12)))
        want = (str(z["chain"][i]).split(">")[0], str(z["chain"][i]), int(z["prologue"][i]), int(z["prologue_bytes"][i]),
                int(z["half_storage"][i]), int(z["half_storage_both"][i]))
        if got != want:
            bad.append((str(z["source"][i]), mode, z["geom"][i][:18].tolist(), got, want))
    assert not bad, f"{len(bad)} of {len(z['mode'])} calls changed kernels, first: {bad[:3]}"


WS = 192 << 20              # what the product offers every launch (ops.WORKSPACE_BYTES)
UNLIMITED = 1 << 62


@pytest.fixture(scope="module")
def shapes(golden_dir):
    """Kernel, grid and reduce of every recorded call's launches, traced on the commit named inside
    (tools/record_conv_launch_shapes.py)."""
    return np.load(os.path.join(golden_dir, "conv_launch_shapes.npz"))


def launch_shape(lib, z, i, precision, step, ws_bytes):
    """conv_launch_shape of step `step` of call i's plan at `precision`; None past the plan's end."""
    ga = (ctypes.c_int * z["geom"].shape[1])(*[int(v) for v in z["geom"][i]])
    sa = (ctypes.c_int64 * 4)(*[int(v) for v in z["strides"][i]])
    ad = (ctypes.c_int64 * 5)(*[int(v) for v in z["addr16"][i]])
    out = (ctypes.c_int64 * 12)()
    n = lib.cpu_launch_shape(ga, sa, int(z["mode"][i]), int(precision), int(z["accumulate"][i]), int(z["has_mask"][i]), ad,
                             step, ctypes.c_uint64(ws_bytes), out)
    if step >= n:
        return None
    keys = ("refuse", "front", "slabs", "splits", "per_split", "gx", "gy", "gz", "tm", "tn", "kernel", "next")
    d = dict(zip(keys, [int(v) for v in out]))
    d["kernel"] = lib.cpu_kernel_name(d["kernel"]).decode()
    return d


def test_every_recorded_launch_gets_the_parents_grid(lib, calls, shapes):
    """At the product's 192 MiB, every step of every recorded chain (and the fp32 variant of every geometry) gets the grid the
    traced commit launched, and splits K exactly where a split-K reduce followed.  Two kernels shape their own launches and
    are held to their name and to taking no split only: the 1x1x1 streaming form in front of the chunked tile kernel (the
    shape is the tile kernel's, which serves where the streaming form refuses the tensors) and Conv3d_1a's persistent tiled
    forward (one workgroup per compute unit of the device)."""
    z, s = calls, shapes
    assert len(s["row"]) > 1000 and len(str(s["commit"])) == 40
    bad, n_own = [], 0
    for j in range(len(s["row"])):
        i, variant, prec = int(s["row"][j]), str(s["variant"][j]), int(s["precision"][j])
        steps = ["vector" if c.startswith("vector") else c.rstrip("*") for c in str(z["chain"][i]).split(">")]
        step = 0 if variant == "fp32" else steps.index(variant)
        sh = launch_shape(lib, z, i, prec, step, WS)
        own = str(s["kernel"][j]).startswith(("conv1x1_stream_kernel", "conv1a_tile_fwd_kernel"))
        n_own += own
        if own:
            got = None if sh is None else (sh["kernel"], sh["refuse"], 0)
            want = (str(s["served"][j]), 0, int(s["reduce"][j]))
        else:
            got = None if sh is None else (sh["kernel"], sh["refuse"], [sh["gx"], sh["gy"], sh["gz"]], int(sh["splits"] > 1))
            want = (str(s["served"][j]), 0, s["grid"][j].tolist(), int(s["reduce"][j]))
        if got != want:
            bad.append((i, variant, str(s["kernel"][j]), got, want))
    assert not bad, f"{len(bad)} of {len(s['row'])} launches changed shape, first: {bad[:3]}"
    assert n_own == 105             # 101 streaming launches, 4 tiled Conv3d_1a forwards: every other one is pinned in full


def test_the_workspace_query_never_undersizes(lib, calls):
    """With exactly otal_conv_workspace_bytes, every step of every recorded call's plan (as recorded, and on fp32 operands)
    takes the splits it takes with unlimited workspace."""
    z = calls
    lib.cpu_workspace_bytes.restype = ctypes.c_uint64
    bad = []
    for i in range(len(z["mode"])):
        ga = (ctypes.c_int * z["geom"].shape[1])(*[int(v) for v in z["geom"][i]])
        sa = (ctypes.c_int64 * 4)(*[int(v) for v in z["strides"][i]])
        mode = int(z["mode"][i])
        need = int(lib.cpu_workspace_bytes(ga, sa, mode))
        for prec in (int(z["precision"][i]), 2 if mode == 1 else 0):
            for step in range(8):
                a, b = launch_shape(lib, z, i, prec, step, need), launch_shape(lib, z, i, prec, step, UNLIMITED)
                if a is None:
                    break
                if (a["refuse"], a["splits"], a["per_split"]) != (b["refuse"], b["splits"], b["per_split"]):
                    bad.append((i, prec, step, a, b, need))
    assert not bad, f"{len(bad)} steps under-sized, first: {bad[:2]}"


def test_fit_splits_edges(lib):
    def fit(want, units, rnd, slab1, ws_bytes, null_ws=0):
        out = (ctypes.c_int64 * 3)()
        lib.cpu_fit_splits(want, units, rnd, ctypes.c_uint64(slab1), null_ws, ctypes.c_uint64(ws_bytes), out)
        return tuple(int(v) for v in out)
    slab = 4096
    assert fit(8, 1000, 32, slab, 1 << 30) == (8, 128, 8 * slab)                    # all of it fits: 1000 / 8 = 125 -> 128
    assert fit(8, 1000, 32, slab, 1 << 30, null_ws=1) == (1, 1024, 0)               # a null workspace holds nothing, whatever its size
    assert fit(8, 1000, 32, slab, slab * 5 // 2) == (2, 512, 2 * slab)              # 2.5 slabs: 2 splits, 1000 / 2 = 500 -> 512
    assert fit(8, 1000, 32, slab, slab * 19 // 10) == (1, 1024, 0)                  # 1.9 slabs: one split, no slab
    assert fit(8, 100, 1, slab, slab * 5 // 2) == (2, 50, 2 * slab)                 # units that need no rounding
    assert fit(7, 224, 32, slab, 1 << 30) == (7, 32, 7 * slab)
    assert fit(6, 224, 32, slab, 1 << 30) == (4, 64, 4 * slab)                      # rounding leaves splits empty: dropped


def test_walking_every_shape_is_clean_under_sanitizers(calls, tmp_path):
    """Host-only soundness: cpu_conv_select.cpp as a stand-alone program under AddressSanitizer and UBSan walks every recorded
    call through conv_launch_shape at 0, 1 byte, the query's size and 192 MiB (integer overflow, shifts, array bounds)."""
    z = calls
    rows = tmp_path / "rows.txt"
    with open(rows, "w") as f:
        for i in range(len(z["mode"])):
            v = [*z["geom"][i], *z["strides"][i], z["mode"][i], z["precision"][i], z["accumulate"][i], z["has_mask"][i], *z["addr16"][i]]
            f.write(" ".join(str(int(x)) for x in v) + "\n")
    exe = str(tmp_path / "walk")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-DCPU_CONV_SELECT_WALK", "-I" + os.path.join(REPO, "opental_amd", "csrc"),
                           os.path.join(HERE, "cpu_conv_select.cpp"), "-o", exe])
    r = subprocess.run([exe, str(rows)], capture_output=True, text=True)
    assert r.returncode == 0 and "shapes" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-2000:])


def test_every_kernel_path_of_the_model_is_pinned(calls):
    heads = {str(c).split(">")[0].rstrip("*") for c in calls["chain"]}
    for k in ("conv1a", "conv1d_tile", "direct", "chunked", "generic", "proj", "conv1a_wgrad", "proj_wgrad", "wgrad_direct",
              "wgrad1x1_wide", "wgrad1d"):
        assert k in heads, k
    assert any(h.startswith("vector") for h in heads)


def test_a_switch_reaches_the_plan(lib, calls):
    """OTAL_CONV_NO1A=1 moves Conv3d_1a's forward off its own kernel (the harness's switches are table defaults otherwise)."""
    z = calls
    rows = [i for i in range(len(z["mode"])) if str(z["chain"][i]).startswith("conv1a") and int(z["mode"][i]) == 0]
    assert rows
    try:
        assert lib.cpu_set_option(b"OTAL_CONV_NO1A", 1) == 0
        for i in rows:
            chain, _ = plan(lib, z, i)
            assert not chain.startswith("conv1a"), chain
    finally:
        lib.cpu_set_option(b"OTAL_CONV_NO1A", 0)
    assert all(plan(lib, z, i)[0].startswith("conv1a") for i in rows)
