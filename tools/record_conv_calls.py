"""Records every otal_conv_fwd / _dgrad / _wgrad call of the model's workloads, for tests/test_conv_select_cpu.py.

    python tools/record_conv_calls.py record OUT.npz      # on the GPU: the calls
    python tools/record_conv_calls.py expect OUT.npz      # on the CPU: adds the expected columns -> tests/golden/conv_calls.npz

`record` runs one eager THUMOS14 training step at b = 8 and at b = 1, one ActivityNet step at b = 2 and one inference batch
(bench.py's models, synthetic clips and bf16 operands) and keeps, per call: the geometry record, the strides, the mode, the precision bits,
accumulate, whether a mask is fused, and each pointer's address mod 16 (x, w, dy, out, mask; 0 where there is none).  The
pair entry points (one kernel each) are not recorded; a pair launch the library refuses shows up as its two single calls.

`expect` asks the kernel choice (opental_amd/csrc/conv_select.h, through tests/cpu_conv_select.cpp with the options' table
defaults) for each distinct call: the chain of kernels, the prologue layout and bytes, and the bf16-storage answers.
"""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
GOLDEN = os.path.join(REPO, "tests", "golden", "conv_calls.npz")
MODES = {"otal_conv_fwd": 0, "otal_conv_dgrad": 1, "otal_conv_wgrad": 2}


def _value(p):
    return int((p.value if isinstance(p, ctypes.c_void_p) else p) or 0)


def _addr(p):
    return _value(p) % 16


class _Recorder:
    """Stands in for the loaded library: the three launch entry points are noted, then called."""

    def __init__(self, real):
        self._real = real
        self.calls = []
        self.source = ""

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if name not in MODES:
            return fn
        mode = MODES[name]

        def call(*args):
            ga, sa = list(args[0]), list(args[1])
            if mode == 0:       # x, w, scale, shift, y, relu, precision, ...
                x, w, dy, out, mask, acc, prec = args[2], args[3], None, args[6], None, 0, args[8]
            elif mode == 1:     # dy, wt, dx, accumulate, mask, scale, precision, ...
                x, w, dy, out, mask, acc, prec = None, args[3], args[2], args[4], args[6], args[5], args[8]
            else:               # x, dy, dw, accumulate, precision, ...
                x, w, dy, out, mask, acc, prec = args[2], None, args[3], args[4], None, args[5], args[6]
            self.calls.append((self.source, ga, sa, mode, int(prec), int(acc), int(_value(mask) != 0),
                               [_addr(x), _addr(w), _addr(dy), _addr(out), _addr(mask)]))
            return fn(*args)
        return call


def record(out):
    import torch
    import bench
    from opental_amd import _lib as L
    from opental_amd.common import ops
    rec = _Recorder(L.lib())
    L._lib = rec
    dev = torch.device("cuda", 0)
    ops.CONV_PRECISION = 1              # bf16 MFMA operands: bench.py's default (--dtype bf16)
    for name, batch in (("thumos_b8", 8), ("thumos_b1", 1)):
        tr = bench.build_trainer(dev)
        clips, targets, scores = bench.synth_batch(batch, 1000, dev)
        rec.source = name
        tr.step(clips, targets, scores)
        torch.cuda.synchronize()
        ops.STEP.reset()
        del tr
    tr = bench.build_anet_trainer(dev)
    clips, targets, scores = bench.synth_batch(2, 1000, dev, frames=768, classes=150, score_rows=3)
    rec.source = "anet_b2"
    tr.step(clips, targets, scores)
    torch.cuda.synchronize()
    ops.STEP.reset()
    del tr
    from opental_amd.thumos14 import test as T
    from opental_amd.thumos14.BDNet import BDNet
    torch.manual_seed(0)
    net = BDNet(training=False, use_edl=True)
    net.backbone._model.apply(BDNet.weight_init)
    net = net.to(dev).eval()
    g = torch.Generator(device=dev).manual_seed(0)
    rec.source = "inference"
    T.detect_batch(net, [torch.randint(0, 256, (3, 700, 96, 96), device=dev, generator=g, dtype=torch.uint8)], 10.0, batch_clips=32)
    torch.cuda.synchronize()
    L._lib = rec._real
    c = rec.calls
    np.savez_compressed(out, source=np.array([r[0] for r in c]), geom=np.array([r[1] for r in c], np.int32),
                        strides=np.array([r[2] for r in c], np.int64), mode=np.array([r[3] for r in c], np.int32),
                        precision=np.array([r[4] for r in c], np.int32), accumulate=np.array([r[5] for r in c], np.int32),
                        has_mask=np.array([r[6] for r in c], np.int32), addr16=np.array([r[7] for r in c], np.int64))
    print(f"{len(c)} calls -> {out}")


def harness():
    """tests/cpu_conv_select.cpp, compiled with g++ (the test builds it the same way)."""
    so = os.path.join(tempfile.mkdtemp(), "libcpuselect.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-std=c++17", "-I" + os.path.join(REPO, "opental_amd", "csrc"),
                           os.path.join(REPO, "tests", "cpu_conv_select.cpp"), "-o", so])
    lib = ctypes.CDLL(so)
    lib.cpu_kernel_name.restype = ctypes.c_char_p
    lib.cpu_prologue_bytes.restype = ctypes.c_int64
    return lib


def ask(lib, geom, strides, mode, precision, accumulate, has_mask, addr16):
    """(chain, prologue layout, prologue bytes, bf16 storage as recorded, with both sides) of one call.  chain: the kernel
    names joined by '>', a '*' after those that move on when they refuse the launch, the vector width after 'vector'."""
    ga = (ctypes.c_int * len(geom))(*[int(v) for v in geom])
    sa = (ctypes.c_int64 * 4)(*[int(v) for v in strides])
    ad = (ctypes.c_int64 * 5)(*[int(v) for v in addr16])
    out = (ctypes.c_int * 32)()
    lib.cpu_conv_plan(ga, sa, int(mode), int(precision), int(accumulate), int(has_mask), ad, out)
    steps = []
    for i in range(out[0]):
        k, cw, nxt = out[2 + 3 * i], out[3 + 3 * i], out[4 + 3 * i]
        steps.append(lib.cpu_kernel_name(k).decode() + (str(cw) if k == 10 else "") + ("*" if nxt else ""))
    return (">".join(steps), int(out[1]), int(lib.cpu_prologue_bytes(ga, sa, int(mode), int(precision))),
            int(lib.cpu_half_storage(ga, sa, int(mode), int(precision))), int(lib.cpu_half_storage(ga, sa, int(mode), int(precision) | 12)))


COLUMNS = ("geom", "strides", "mode", "precision", "accumulate", "has_mask", "addr16")


def expect(raw):
    z = np.load(raw)
    # one row per distinct call (the same layer shape recurs across steps and recipes): the first source that made it
    seen, keep = set(), []
    for i in range(len(z["mode"])):
        key = tuple(np.concatenate([np.asarray(z[c][i]).ravel() for c in COLUMNS]).tolist())
        if key not in seen:
            seen.add(key)
            keep.append(i)
    cols = {c: z[c][keep] for c in ("source",) + COLUMNS}
    lib = harness()
    ans = [ask(lib, *(cols[c][j] for c in COLUMNS)) for j in range(len(keep))]
    np.savez_compressed(GOLDEN, **cols, chain=np.array([a[0] for a in ans]), prologue=np.array([a[1] for a in ans], np.int32),
                        prologue_bytes=np.array([a[2] for a in ans], np.int64), half_storage=np.array([a[3] for a in ans], np.int32),
                        half_storage_both=np.array([a[4] for a in ans], np.int32))
    print(f"{len(z['mode'])} calls, {len(keep)} distinct -> {GOLDEN}")


if __name__ == "__main__":
    {"record": record, "expect": expect}[sys.argv[1]](sys.argv[2])
