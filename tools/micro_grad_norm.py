"""What the global gradient norm costs the training step: python tools/micro_grad_norm.py [--batch 8] [--steps 20] [--runs 7]
[--variants off,track,clip] [--clip 20] [--lib ab/<name>.so --header <that commit's opental_hip.h>]

In ONE process on one GPU, at bf16 operands with the ssl branch off (the benchmark's configuration):
  * the norm launch alone (otal_grad_norm: partial sums + finish) over a buffer of the flat arena's size, next to the Adam
    launch (otal_adam_flat_dev) over the same elements -- HIP events around `reps` launches, median over the runs;
  * the resident replayed lane-graph step (inputs already in the captured step's buffers) three ways: flags off, tracking
    (DetectorTrainer.track_grad_norm), clipping (clip_grad_norm = --clip; the captured step gives up the early Adam).
The step variants ALTERNATE, `--runs` times, `--steps` steps per window after warm-up; a window is a host clock around work
that ends in a device synchronise.  Printed: median and min .. max over the runs (ms per step).

--lib / --header: time `--variants off` on the library of another commit (tools/build_lib_at.sh <commit> <name>; the header
is `git show <commit>:include/opental_hip.h`, from which the ctypes signatures of THAT library are read) -- the parent's
step on the same box, in the same job, alternating with this one."""
import functools
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def arg(name, default, kind=int):
    return kind(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


if "--lib" in sys.argv:             # before the package binds the library
    os.environ["OTAL_LIB_PATH"] = os.path.abspath(arg("--lib", None, str))
import bench  # noqa: E402
from opental_amd import _lib as L  # noqa: E402
from opental_amd.common import ops  # noqa: E402

if "--header" in sys.argv:
    L.signatures = functools.partial(L.signatures, os.path.abspath(arg("--header", None, str)))


def window(tr, n):
    clips, targets, scores = tr.static_inputs()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        tr.step(clips, targets, scores)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def launches(n, dev, runs, reps=20):
    """ms per call of the norm launch and of the Adam launch over n elements."""
    g = torch.randn(n, dtype=torch.float32, device=dev)
    p, m, v = torch.randn_like(g), torch.zeros_like(g), torch.zeros_like(g)
    bc = torch.tensor(ops.adam_bias_corrections(3), dtype=torch.float32, device=dev)
    out = torch.zeros(2, dtype=torch.float32, device=dev)
    res = {}
    calls = [("otal_adam_flat_dev", 28 * n, lambda: ops.adam_flat_dev(p, g, m, v, bc, 1e-5, weight_decay=1e-3))]
    if hasattr(ops, "grad_norm") and "--lib" not in sys.argv:
        ws = torch.zeros(ops.GRAD_NORM_PARTIALS, dtype=torch.float64, device=dev)
        calls.insert(0, ("otal_grad_norm", 4 * n, lambda: ops.grad_norm(g, 1.0, 20.0, out, ws)))
        calls.append(("otal_adam_flat_clip", 28 * n, lambda: ops.adam_flat_clip(p, g, m, v, bc, out, 1e-5, weight_decay=1e-3)))
    for name, nbytes, fn in calls:
        for _ in range(5):
            fn()
        ms = []
        for _ in range(runs):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b) / reps)
        res[name] = (ms, nbytes)
    return res


def main():
    batch, steps, runs = arg("--batch", 8), arg("--steps", 20), arg("--runs", 7)
    clip = arg("--clip", 20.0, float)
    names = arg("--variants", "off,track,clip", str).split(",")
    if not torch.cuda.is_available():
        raise SystemExit("micro_grad_norm needs an MI355X")
    dev = torch.device("cuda", 0)
    ops.CONV_PRECISION = 1
    batch_in = bench.synth_batch(batch, 1000, dev)
    trainers = {}
    for name in names:
        tr = bench.build_trainer(dev)
        if name == "track":
            tr.track_grad_norm = True
        elif name == "clip":
            tr.clip_grad_norm = clip
        elif name != "off":
            raise SystemExit("--variants takes off, track, clip")
        tr.capture_step(*batch_in, warmup=2, lanes=True)
        window(tr, 5)
        assert tr.replayed_steps >= 5, name + ": the step did not replay"
        trainers[name] = tr
    times = {name: [] for name in names}
    for _ in range(runs):
        for name in names:                          # alternating: drift of the shared host hits every variant alike
            times[name].append(window(trainers[name], steps))
    lib = os.environ.get("OTAL_LIB_PATH", "this tree's library")
    print(f"{lib}: b = {batch}, bf16 operands, ssl off, {runs} runs x {steps} replayed lane-graph steps per variant "
          "(ms per step: median, min .. max)")
    for name in names:
        t = times[name]
        extra = ""
        if name != "off" and trainers[name].last_grad_norm is not None:
            extra = "   last {norm, coef} = " + str([round(x, 5) for x in trainers[name].last_grad_norm.tolist()])
        print(f"  {name:6s} {statistics.median(t):8.3f}  {min(t):8.3f} .. {max(t):8.3f}{extra}", flush=True)
    n = next(iter(trainers.values())).arena.numel
    for name, (ms, nbytes) in launches(n, dev, runs).items():
        med = statistics.median(ms)
        print(f"  {name:20s} n = {n}: {med * 1e3:8.1f} us  {min(ms) * 1e3:8.1f} .. {max(ms) * 1e3:8.1f}   "
              f"{nbytes / med / 1e9:6.2f} TB/s of {nbytes / 1e6:.0f} MB", flush=True)


if __name__ == "__main__":
    main()
