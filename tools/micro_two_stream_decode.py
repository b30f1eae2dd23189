"""Times the glue between the two networks of a two-stream THUMOS14 run and the decode launch, on the GPU, both routes in one
process on the same raw outputs: from the per-chunk raw output maps of the rgb and the flow network to the `dec` dict that
Soft-NMS reads.
  fused     : the earlier route (detect_batch(two_stream_decode=False)) -- fuse_outputs per chunk of windows, the averaged maps
              concatenated, decode_clips, the uncertainty substituted by ((unct + prop_unct) / 2).contiguous();
  two_stream: the default route -- each network's maps concatenated, decode_clips_two_stream (otal_decode_clips_2s).
One batch of the test loop: --videos 8 videos of --frames 2048 sampled frames (15 windows each, 120 clips in chunks of 32),
A = 126 anchors, K = 15 classes, the OpenTAL head.  The maps are random (the glue does not care what the networks computed);
every run starts from the same per-chunk tensors.  Host clocks around device synchronisations, the two routes alternating,
the median of --runs runs after --warmup warm-ups; the device launches of one call of each route are counted from a
torch.profiler trace taken outside the timed runs.  The two routes' dec tensors must be torch.equal.

    python tools/micro_two_stream_decode.py [--videos 8] [--frames 2048] [--runs 200] [--warmup 20] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np
import torch

KEYS = ('loc', 'conf', 'prop_loc', 'prop_conf', 'center', 'priors', 'act', 'prop_act', 'unct', 'prop_unct')


def chunk_outputs(g, n, A, K, priors):
    """What one forward pass of one network over n windows hands the glue."""
    r = lambda *s: torch.randn(*s, device='cuda', generator=g)
    u = lambda *s: torch.rand(*s, device='cuda', generator=g) * 0.9 + 0.05
    return dict(loc=r(n, A, 2) * 40.0, prop_loc=r(n, A, 2), conf=r(n, A, K) * 2.0, prop_conf=r(n, A, K) * 2.0, center=r(n, A, 1),
                act=r(n, A, 1), prop_act=r(n, A, 1), unct=u(n, A), prop_unct=u(n, A), priors=priors)


def merge(parts):
    return {k: (torch.cat([o[k] for o in parts], 0) if k != 'priors' else parts[0][k]) for k in KEYS}


def count_launches(fn):
    """Device kernels of one call, from a profiler trace (copies and memsets are not launches of ours)."""
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == DeviceType.CUDA
             and not any(w in e.name.lower() for w in ('memcpy', 'memset', 'copybuffer', 'fillbuffer'))]
    return len(names), names


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--videos', type=int, default=8)
    p.add_argument('--frames', type=int, default=2048)
    p.add_argument('--runs', type=int, default=200)
    p.add_argument('--warmup', type=int, default=20)
    p.add_argument('--out', type=str, default=None)
    args = p.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("micro_two_stream_decode.py measures on the GPU; none found")
    from opental_amd.common import detect as D
    A, K, clip_length, stride, conf_thresh = 126, 15, 256, 128, 0.01
    per_video = len(D.get_offsets(args.frames, clip_length, stride))
    n = args.videos * per_video
    offsets = [float(o) for _ in range(args.videos) for o in D.get_offsets(args.frames, clip_length, stride)]
    fps = [10.0] * n
    g = torch.Generator(device='cuda').manual_seed(0)
    priors = ((torch.arange(A, device='cuda', dtype=torch.float32) + 0.5) / A).view(A, 1)
    step = D.windows_per_pass(32)
    sizes = [min(step, n - i) for i in range(0, n, step)]
    rgb = [chunk_outputs(g, m, A, K, priors) for m in sizes]
    flow = [chunk_outputs(g, m, A, K, priors) for m in sizes]

    def fused():
        merged = merge([D.fuse_outputs(a, b) for a, b in zip(rgb, flow)])
        dec = D.decode_clips(merged, offsets, fps, clip_length, conf_thresh)
        dec['unct'] = ((merged['unct'] + merged['prop_unct']) / 2.0).contiguous()
        return dec

    def two_stream():
        return D.decode_clips_two_stream(merge(rgb), merge(flow), offsets, fps, clip_length, conf_thresh)

    routes = dict(fused=fused, two_stream=two_stream)
    a, b = fused(), two_stream()
    torch.cuda.synchronize()
    for k in a:
        if not torch.equal(a[k], b[k]):
            raise SystemExit(f"the two routes disagree on dec['{k}']")
    flagged = int(a['flag'].sum())
    times = {k: [] for k in routes}
    for it in range(args.warmup + args.runs):
        for name, fn in routes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if it >= args.warmup:
                times[name].append(dt * 1e6)
    launches = {}
    for name, fn in routes.items():
        try:
            launches[name] = count_launches(fn)[0]
        except Exception as e:          # a profiler that cannot trace here: the times stand, the count is not measured
            launches[name] = f"not measured ({type(e).__name__}: {e})"
    stats = lambda v: dict(median=float(np.median(v)), p10=float(np.percentile(v, 10)), p90=float(np.percentile(v, 90)))
    result = dict(videos=args.videos, clips=n, chunks=sizes, A=A, K=K, flagged=flagged, runs=args.runs, warmup=args.warmup,
                  call_us={k: stats(v) for k, v in times.items()}, launches=launches,
                  two_stream_over_fused=float(np.median(times['two_stream']) / np.median(times['fused'])))
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + "\n")
    return result


if __name__ == '__main__':
    main()
