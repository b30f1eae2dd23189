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
