"""What the non-finite-gradient guard costs the training step: python tools/micro_nonfinite_guard.py [--batch 8] [--steps 20]
[--runs 7] [--variants off,clip,guard] [--clip 20]

In ONE process on one GPU, at bf16 operands with the ssl branch off (the benchmark's configuration):
  * the resident replayed lane-graph step (inputs already in the captured step's buffers) three ways: flags off, clipping
    (clip_grad_norm = --clip: the other feature that gives up the early Adam, for comparison on the same box), the guard
    (DetectorTrainer.skip_nonfinite);
  * the gate launch alone (otal_step_gate, one workgroup, with a 50-float loss state), and the Adam sweep over the flat arena's
    size three ways: otal_adam_flat_sched, otal_adam_flat_guard applied, otal_adam_flat_guard skipped (the empty launch) --
    HIP events around `reps` launches, median over the runs.
The step variants ALTERNATE, `--runs` times, `--steps` steps per window after warm-up; a window is a host clock around work
that ends in a device synchronise.  Printed: median and min .. max over the runs (ms per step), and each variant's ratio to
`off`."""
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import bench  # noqa: E402
from opental_amd.common import ops  # noqa: E402
from opental_amd.common import step_guard as G  # noqa: E402


def arg(name, default, kind=int):
    return kind(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def window(tr, n):
    clips, targets, scores = tr.static_inputs()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        tr.step(clips, targets, scores)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def record(dev, apply):
    r = G.new_record(3, 0)
    r['apply'] = apply
    return torch.from_numpy(np.frombuffer(r.tobytes(), dtype=np.int64).copy()).to(dev)


def launches(n, dev, runs, reps=20):
    """ms per call of the gate and of the three Adam sweeps over n elements."""
    g = torch.randn(n, dtype=torch.float32, device=dev)
    p, m, v = torch.randn_like(g), torch.zeros_like(g), torch.zeros_like(g)
    ss = torch.tensor(ops.adam_bias_corrections(3) + [1.0, 0.0], dtype=torch.float32, device=dev)
    norm = torch.tensor([1.0, 1.0], dtype=torch.float32, device=dev)
    gate_rec, on, off = record(dev, 1), record(dev, 1), record(dev, 0)
    made = torch.zeros(4, dtype=torch.float32, device=dev)
    state, keep = torch.ones(50, device=dev), torch.ones(50, device=dev)
    calls = [("otal_step_gate", 0, lambda: ops.step_gate(norm, gate_rec, made, host_state=ss, loss_state=state, loss_state_keep=keep)),
             ("otal_adam_flat_sched", 28 * n, lambda: ops.adam_flat_sched(p, g, m, v, ss, 1e-5, weight_decay=1e-3)),
             ("otal_adam_flat_guard applied", 28 * n, lambda: ops.adam_flat_guard(p, g, m, v, ss, on, 1e-5, weight_decay=1e-3)),
             ("otal_adam_flat_guard skipped", 0, lambda: ops.adam_flat_guard(p, g, m, v, ss, off, 1e-5, weight_decay=1e-3))]
    res = {}
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
    names = arg("--variants", "off,clip,guard", str).split(",")
    if not torch.cuda.is_available():
        raise SystemExit("micro_nonfinite_guard needs an MI355X")
    dev = torch.device("cuda", 0)
    ops.CONV_PRECISION = 1
    batch_in = bench.synth_batch(batch, 1000, dev)
    trainers = {}
    for name in names:
        tr = bench.build_trainer(dev)
        if name == "clip":
            tr.clip_grad_norm = clip
        elif name == "guard":
            tr.skip_nonfinite = True
        elif name != "off":
            raise SystemExit("--variants takes off, clip, guard")
        tr.capture_step(*batch_in, warmup=2, lanes=True)
        window(tr, 5)
        assert tr.replayed_steps >= 5, name + ": the step did not replay"
        trainers[name] = tr
    times = {name: [] for name in names}
    for _ in range(runs):
        for name in names:                          # alternating: drift of the shared host hits every variant alike
            times[name].append(window(trainers[name], steps))
    print(f"b = {batch}, bf16 operands, ssl off, {runs} runs x {steps} replayed lane-graph steps per variant "
          "(ms per step: median, min .. max, median / off)")
    base = statistics.median(times["off"]) if "off" in times else None
    for name in names:
        t = times[name]
        extra = "" if base is None else f"   x{statistics.median(t) / base:.4f}"
        if name == "guard":
            extra += "   (applied, nonfinite) = " + str(trainers[name].guard_counts())
        print(f"  {name:6s} {statistics.median(t):8.3f}  {min(t):8.3f} .. {max(t):8.3f}{extra}", flush=True)
    n = next(iter(trainers.values())).arena.numel
    for name, (ms, nbytes) in launches(n, dev, runs).items():
        med = statistics.median(ms)
        rate = f"   {nbytes / med / 1e9:6.2f} TB/s of {nbytes / 1e6:.0f} MB" if nbytes else ""
        print(f"  {name:30s} n = {n}: {med * 1e3:8.1f} us  {min(ms) * 1e3:8.1f} .. {max(ms) * 1e3:8.1f}{rate}", flush=True)


if __name__ == "__main__":
    main()
