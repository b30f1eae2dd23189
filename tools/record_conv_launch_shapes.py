"""Records the launch every recorded convolution call gets -- kernel, grid, split-K reduce or not -- for
tests/test_conv_select_cpu.py, which holds conv_launch_shape() (opental_amd/csrc/conv_select.h) to it.

    timeout -k 10 900 rocprofv3 --kernel-trace --output-format csv -d DIR -o replay -- \
        python tools/record_conv_launch_shapes.py replay DIR/manifest.json       # on the GPU, under a time limit
    python tools/record_conv_launch_shapes.py collect DIR/manifest.json TRACE.csv COMMIT
                                                             # anywhere: -> tests/golden/conv_launch_shapes.npz

`replay` sends each row of tests/golden/conv_calls.npz through the C ABI the way tests/test_conv_calls_gpu.py does (its
operands, its launch(), table-default options, 192 MiB of workspace): every step of the row's chain, the later ones
reached by the switches that remove the steps before them, and the fp32 variant once per geometry.  Before each call, and
after the last, it launches a marker (an integer xor: no kernel of the library's).  With `--hash` it also keeps a SHA-256 of
each call's raw output buffer, to compare two builds of the library byte for byte.

`collect` cuts the kernel trace at the markers.  Per call it keeps the last kernel of the library's that is not a split-K
reduction (tables and weight packs come before it), its grid in workgroups (the trace counts work-items) and whether a
reduction followed.  COMMIT is the commit the traced library was built from.
"""
import csv
import glob
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
GOLDEN = os.path.join(REPO, "tests", "golden", "conv_launch_shapes.npz")
MARKER = re.compile(r"bitwise_?xor", re.I)


def items(T):
    """(row, variant, switches, precision) of every replayed call: test_conv_calls_gpu's chain-step and fp32 variants."""
    out = []
    for i, name, switches, prec in T.VARIANTS:
        steps = [T.kname(s) for s in T.chain_steps(i)]
        if name == "fp32" or (name in steps and len(switches) == steps.index(name)):
            out.append((i, name, switches, int(T.Z["precision"][i]) if prec is None else prec))
    return out


def replay(manifest, want_hash):
    import torch
    import test_conv_calls_gpu as T
    from opental_amd import _lib as L
    lib = L.lib()
    for n, d in T.OPTIONS:
        L.set_option(n, d)
    so = os.path.join(tempfile.mkdtemp(), "libcpuselect.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-std=c++17", "-I" + os.path.join(REPO, "opental_amd", "csrc"),
                           os.path.join(REPO, "tests", "cpu_conv_select.cpp"), "-o", so])
    import ctypes
    H = ctypes.CDLL(so)
    H.cpu_kernel_name.restype = ctypes.c_char_p
    mark = torch.zeros(64, dtype=torch.int32, device="cuda")
    one = torch.ones(64, dtype=torch.int32, device="cuda")
    calls = []
    for i, name, switches, prec in items(T):
        row = T.get_row(i)
        plan = T.cpu_plan(H, i, prec, switches)
        T.set_switches(switches, True)
        try:
            torch.cuda.synchronize()
            mark.bitwise_xor_(one)
            rc, got, obase, off, o_half, ws = T.launch(lib, row, prec)
        finally:
            T.set_switches(switches, False)
        call = {"row": i, "variant": name, "precision": prec, "switches": list(switches), "rc": int(rc), "served": got,
                "plan": plan}
        if want_hash:
            raw = obase.view(torch.int16 if o_half else torch.int32).cpu().numpy()
            call["sha256"] = hashlib.sha256(raw.tobytes()).hexdigest()
        calls.append(call)
        del obase, ws
        if len(calls) % 50 == 0:
            print(f"{len(calls)} calls", flush=True)
    mark.bitwise_xor_(one)
    torch.cuda.synchronize()
    with open(manifest, "w") as f:
        json.dump(calls, f)
    print(f"{len(calls)} calls -> {manifest}")


def library_kernels():
    names = set()
    for path in glob.glob(os.path.join(REPO, "opental_amd", "csrc", "*")):
        if path.endswith((".hip", ".inc", ".h")):
            names.update(re.findall(r"__global__[^;{]*?\bvoid\s+(\w+)\s*\(", open(path).read()))
    return names


def collect(manifest, trace, commit):
    calls = json.load(open(manifest))
    rows = sorted(csv.DictReader(open(trace)), key=lambda r: int(r["Dispatch_Id"]))
    ours = re.compile(r"\b(" + "|".join(sorted(library_kernels())) + r")\b(<[^(]*>)?")
    segments, cur = [], None
    for r in rows:
        name = r["Kernel_Name"]
        if MARKER.search(name):
            cur = []
            segments.append(cur)
        elif cur is not None:
            m = ours.search(name)
            if m:
                grid = tuple(int(r["Grid_Size_" + c]) // max(int(r["Workgroup_Size_" + c]), 1) for c in "XYZ")
                cur.append((m.group(1), (m.group(1) + (m.group(2) or "")).replace(" ", ""), grid))
    assert len(segments) == len(calls) + 1, (len(segments), len(calls))
    assert not segments[-1], segments[-1]
    cols = {k: [] for k in ("row", "variant", "precision", "served", "kernel", "grid", "reduce")}
    for c, seg in zip(calls, segments):
        assert c["rc"] == 0 and c["served"] == c["plan"][0], c
        main = [k for k in seg if "splitk_reduce" not in k[0]]
        assert main, c
        cols["row"].append(c["row"])
        cols["variant"].append(c["variant"])
        cols["precision"].append(c["precision"])
        cols["served"].append(c["served"])
        cols["kernel"].append(main[-1][1])
        cols["grid"].append(main[-1][2])
        cols["reduce"].append(int(len(main) < len(seg)))
    np.savez_compressed(GOLDEN, commit=np.array(commit), row=np.array(cols["row"], np.int32), variant=np.array(cols["variant"]),
                        precision=np.array(cols["precision"], np.int32), served=np.array(cols["served"]),
                        kernel=np.array(cols["kernel"]), grid=np.array(cols["grid"], np.int64),
                        reduce=np.array(cols["reduce"], np.int32))
    print(f"{len(calls)} launches ({sum(cols['reduce'])} with a reduce) -> {GOLDEN}")


if __name__ == "__main__":
    if sys.argv[1] == "replay":
        replay(sys.argv[2], "--hash" in sys.argv[3:])
    else:
        collect(sys.argv[2], sys.argv[3], sys.argv[4])
