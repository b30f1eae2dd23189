"""What the learning-rate schedule and the weight EMA cost: python tools/micro_lr_ema.py [--batch 8] [--steps 20] [--runs 7]
[--n 44700000] [--variants off,sched_ema] [--kernels-only] [--lib ab/<name>.so --header <that commit's opental_hip.h>]

In ONE process on one GPU:
  * the Adam sweep over `--n` elements (default: the flat arena's 44.7 M) three ways, ALTERNATING, HIP events around `reps`
    launches, median and min .. max over the runs, achieved bytes/s:
      (a) otal_adam_flat_dev                                    7 floats per parameter
      (b) otal_adam_flat_sched with the EMA                     9 floats per parameter, one launch
      (c) otal_adam_flat_dev, then torch.lerp_ on an EMA array  7 + 3 floats per parameter, two launches
  * the resident replayed lane-graph step at bf16 operands with the ssl branch off (the benchmark's configuration), flags off
    and with a cosine schedule + EMA, alternating, `--steps` steps per window; a window is a host clock around work that ends
    in a device synchronise.

--lib / --header: time `--variants off` on the library of another commit (tools/build_lib_at.sh <commit> <name>), as
tools/micro_grad_norm.py does -- the parent's step on the same box."""
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


def kernels(n, dev, runs, reps=20):
    """{name: (ms per call over the runs, bytes moved)} of the three Adam routes over n elements, alternating."""
    from opental_amd.common import lr_schedule as S
    g = torch.randn(n, dtype=torch.float32, device=dev)
    p, m, v = torch.randn_like(g), torch.zeros_like(g), torch.zeros_like(g)
    ema = p.clone()
    keep = float(S.ema_keep(0.999, 3))
    rec = torch.tensor(S.step_state(ops.adam_bias_corrections(3), 0.75, keep).tolist(), dtype=torch.float32, device=dev)

    def separate():
        ops.adam_flat_dev(p, g, m, v, rec, 1e-5, weight_decay=1e-3)
        ema.lerp_(p, 1.0 - keep)
    calls = [("(a) adam_flat_dev", 28 * n, lambda: ops.adam_flat_dev(p, g, m, v, rec, 1e-5, weight_decay=1e-3))]
    if hasattr(ops, "adam_flat_sched") and "--lib" not in sys.argv:
        calls.append(("(b) adam_flat_sched + ema", 36 * n, lambda: ops.adam_flat_sched(p, g, m, v, rec, 1e-5, weight_decay=1e-3, ema=ema)))
        calls.append(("    adam_flat_sched, no ema", 28 * n, lambda: ops.adam_flat_sched(p, g, m, v, rec, 1e-5, weight_decay=1e-3)))
    calls.append(("(c) adam_flat_dev + lerp_", 40 * n, separate))
    res = {name: ([], nbytes) for name, nbytes, _ in calls}
    for _, _, fn in calls:
        for _ in range(5):
            fn()
    for _ in range(runs):
        for name, _, fn in calls:                   # alternating: drift of the shared box hits every variant alike
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            b.synchronize()
            res[name][0].append(a.elapsed_time(b) / reps)
    return res


def main():
    batch, steps, runs = arg("--batch", 8), arg("--steps", 20), arg("--runs", 7)
    names = arg("--variants", "off,sched_ema", str).split(",")
    if not torch.cuda.is_available():
        raise SystemExit("micro_lr_ema needs an MI355X")
    dev = torch.device("cuda", 0)
    ops.CONV_PRECISION = 1
    n = arg("--n", 44_700_000)
    for name, (ms, nbytes) in kernels(n, dev, runs).items():
        med = statistics.median(ms)
        print(f"  {name:28s} n = {n}: {med * 1e3:8.1f} us  {min(ms) * 1e3:8.1f} .. {max(ms) * 1e3:8.1f}   "
              f"{nbytes / med / 1e9:6.2f} TB/s of {nbytes / 1e6:.0f} MB", flush=True)
    if "--kernels-only" in sys.argv:
        return
    batch_in = bench.synth_batch(batch, 1000, dev)
    trainers = {}
    for name in names:
        tr = bench.build_trainer(dev)
        if name == "sched_ema":
            tr.lr_schedule = dict(name="cosine", total_steps=100000, warmup_steps=1000, min_lr_ratio=0.01)
            tr.ema_decay = 0.999
        elif name != "off":
            raise SystemExit("--variants takes off, sched_ema")
        tr.capture_step(*batch_in, warmup=2, lanes=True)
        window(tr, 5)
        assert tr.replayed_steps >= 5, name + ": the step did not replay"
        trainers[name] = tr
    times = {name: [] for name in names}
    for _ in range(runs):
        for name in names:
            times[name].append(window(trainers[name], steps))
    lib = os.environ.get("OTAL_LIB_PATH", "this tree's library")
    print(f"{lib}: b = {batch}, bf16 operands, ssl off, {runs} runs x {steps} replayed lane-graph steps per variant "
          "(ms per step: median, min .. max)")
    for name in names:
        t = times[name]
        print(f"  {name:10s} {statistics.median(t):8.3f}  {min(t):8.3f} .. {max(t):8.3f}   arena {trainers[name].arena.numel} elements",
              flush=True)


if __name__ == "__main__":
    main()
