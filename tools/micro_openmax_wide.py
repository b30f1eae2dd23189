"""Times the wide OpenMax decode launch (otal_decode_clips_openmax_wide, csrc/openmax_wide.hip) at the ActivityNet shape --
K = 150 classes, A = 189 anchors, D = 512 -- for n in {4, 32} clips and rank R in {1, 3}, with and without the refined
feature, and beside it the float32 numpy restatement of the same arithmetic on the host (tests/openmax_ref.py: every
distance, which is also what the reference's per-anchor, per-class Python loop computes).

    python tools/micro_openmax_wide.py [--json FILE] [--clips N] [--rank R]

`--clips` / `--rank` restrict the run to one shape, for kernel-only time under `tools/kernel_time.sh 4 -- python
tools/micro_openmax_wide.py --clips 32 --rank 1` (rocprofv3 --kernel-trace --stats; in a run of its own: tracing slows the host).

Device time: HIP events round a window of back-to-back launches, after a warm-up of the same shape; the window is sized to
last at least 0.2 s and is repeated 5 times (median and spread are printed).  Host time: wall clock round one evaluation
(its fastest of 3).  Needs a GPU: there is no fallback."""
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import openmax_ref as R
import openmax_wide_ref as W
from opental_amd.anet.openmax import OpenMax, WeibullFit
from opental_amd.anet.test_openmax import decode_clips_openmax

K, D, A = W.K, W.D, W.A


def inputs(n, seed=1):
    cen, pcen = R.class_centres(seed, K, D), R.class_centres(seed + 1, K, D)
    outs = W.clip_outputs(seed + 2, cen, pcen, n)
    rs = np.random.RandomState(seed + 3)
    fits = [dict(scale=10000.0 + rs.uniform(0.02, 0.2, K), shape=rs.uniform(1.5e5, 4e5, K), small=rs.uniform(0.08, 0.2, K))
            for _ in range(2)]
    return cen, pcen, outs, fits


def layer(mav, fits, rank, dev):
    model = {f"c{k}": {'mean_vec': mav[k], 'model': [WeibullFit(fits['scale'][k], fits['shape'][k], fits['small'][k])]}
             for k in range(K)}
    return OpenMax(model, rank=rank).to(dev)


def device_time(fn, min_window=0.2, windows=5):
    """Median and (min, max) seconds per call over `windows` event-timed windows of back-to-back calls."""
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    calls = max(20, int(min_window / max((time.perf_counter() - t0) / 20, 1e-7)))
    per = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        per.append(a.elapsed_time(b) * 1e-3 / calls)
    return float(np.median(per)), (min(per), max(per)), calls


def main():
    assert torch.cuda.is_available(), "micro_openmax_wide needs a GPU"
    dev = torch.device("cuda", 0)
    rows = []
    only = lambda flag, all_: (int(sys.argv[sys.argv.index(flag) + 1]),) if flag in sys.argv else all_
    for n in only("--clips", (4, 32)):
        cen, pcen, outs, fits = inputs(n)
        t = {k: torch.from_numpy(v).to(dev) for k, v in outs.items()}
        t['priors'] = torch.from_numpy(W.priors()).to(dev)
        fps = [10.0] * n
        for rank in only("--rank", (1, 3)):
            lay = layer(cen, fits[0], rank, dev), layer(pcen, fits[1], rank, dev)
            host = []
            for _ in range(3):
                t0 = time.perf_counter()
                W.decode(outs, cen, fits[0], pcen, fits[1], rank=rank, dt=np.float32)
                host.append(time.perf_counter() - t0)
            for refined in (False, True):
                med, (lo, hi), calls = device_time(lambda: decode_clips_openmax(t, fps, lay[0], lay[1], 768.0, 0.001, refined))
                rows.append(dict(n=n, rank=rank, refined=refined, device_us=med * 1e6, device_us_min=lo * 1e6,
                                 device_us_max=hi * 1e6, calls_per_window=calls, host_numpy_f32_s=min(host)))
                print(f"n = {n:2d} clips ({n * A} rows), R = {rank}, refined_feature = {int(refined)}: decode call "
                      f"{med * 1e6:8.1f} us (min {lo * 1e6:.1f}, max {hi * 1e6:.1f}; {calls} calls per window, launch and the "
                      f"Python wrapper included); float32 numpy restatement on the host {min(host) * 1e3:8.1f} ms", flush=True)
    if "--json" in sys.argv:
        path = sys.argv[sys.argv.index("--json") + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
