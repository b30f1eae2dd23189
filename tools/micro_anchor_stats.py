"""Times the anchor-statistics pass (opental_amd/common/anchor_stats.py) over a test-split-sized set of windows, in one process,
the host way against the kernel, on the same synthetic head outputs (K = 126, C = 15; the network is not part of either):
  host:   what the reference's analysis scripts do after inference -- every head output copied to the host, then a loop over
          the windows in torch-CPU (the package's torch matching, MultiSegmentLoss.match, then the score and the EDL gradient
          of the window) and numpy histograms at the end;
  kernel: one otal_anchor_stats launch per batch of --batch windows into device histograms, one copy of those at the end.
Host clocks around device synchronisations; the median of --runs runs after --warmup warm-ups.  --windows defaults to 3400,
the order of the THUMOS14 test split at stride 128 (about 210 annotated videos of ~16 windows); pass the real count if known.
The two histograms are compared: on unconstrained random inputs a score within a float32 rounding of a bin edge may be
counted next door by one of the two, so the tool reports the number of counts that differ instead of refusing.

    python tools/micro_anchor_stats.py [--windows 3400] [--batch 128] [--target half_au] [--runs 5] [--warmup 2] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time
import types

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np
import torch

K, C, G, CLIP, OVERLAP, BINS = 126, 15, 4, 256.0, 0.5, 100
LEVELS = (64, 32, 16, 8, 4, 2)


def host_pass(heads, priors, gt, gvalid, target):
    """The per-window loop in torch-CPU -> (hist_score (2, 3, BINS), hist_grad (2, BINS))."""
    from opental_amd.common.anchor_stats import grad_edges
    from opental_amd.thumos14.multisegment_loss import MultiSegmentLoss
    h = {k: v.cpu() for k, v in heads.items()}                      # every head output comes to the host
    gt, gvalid, priors = gt.cpu(), gvalid.cpu().bool(), priors.cpu().view(-1, 1)
    matcher = types.SimpleNamespace(clip_length=CLIP, overlap_thresh=OVERLAP)      # MultiSegmentLoss.match reads these two
    vals = [[[] for _ in range(3)] for _ in range(2)]
    norms = [[], []]
    for w in range(h['loc'].shape[0]):
        t = gt[w][gvalid[w]]
        if t.shape[0]:
            _, conf_t, _, prop_t, _ = MultiSegmentLoss.match(matcher, h['loc'][w:w + 1], priors, [t])
            conf_t, prop_t = conf_t[0], prop_t[0]
        else:
            conf_t = prop_t = torch.zeros(K, dtype=torch.long)
        for s, (lab, zk, ak) in enumerate(((conf_t, 'conf', 'act'), (prop_t, 'prop_conf', 'prop_act'))):
            alpha = torch.exp(torch.clamp(h[zk][w], -10, 10)) + 1
            S = alpha.sum(-1)
            u = C / S
            act = h[ak][w].view(-1).sigmoid()
            if target == 'uncertainty':
                v = u
            elif target == 'actionness':
                v = act
            elif target == 'confidence':
                v = (alpha / S[:, None] * h['center'][w].view(-1, 1).sigmoid() * act[:, None]).max(-1)[0]
            elif target == 'uncertainty_actionness':
                v = u * act
            else:
                v = 0.5 * (act + 1.0) * u
            v = v.numpy()
            vals[s][0].append(v[((lab > 0) & (lab <= C)).numpy()])
            vals[s][1].append(v[(lab > C).numpy()])
            vals[s][2].append(v[(lab == 0).numpy()])
            keep = (lab > 0) & (lab <= C)
            if keep.any():
                y = torch.eye(C)[lab[keep] - 1]
                norms[s].append(((1 / alpha[keep] - u[keep, None]) * y).abs().sum(-1).numpy())
    hist_score = np.zeros((2, 3, BINS), np.int64)
    hist_grad = np.zeros((2, BINS), np.int64)
    edges = grad_edges(BINS)
    for s in range(2):
        for g in range(3):
            v = np.concatenate(vals[s][g]) if vals[s][g] else np.zeros(0, np.float32)
            hist_score[s, g] = np.bincount(np.minimum(np.floor(v * np.float32(BINS)), BINS - 1).astype(np.int64), minlength=BINS)
        n = np.concatenate(norms[s]) if norms[s] else np.zeros(0, np.float32)
        for i in range(BINS):
            hist_grad[s, i] = ((n >= edges[i]) & (n < edges[i + 1])).sum()
    return hist_score, hist_grad


def kernel_pass(heads, priors, gt, gvalid, target, batch):
    from opental_amd.common import ops
    dev = heads['loc'].device
    out = dict(hist_score=torch.zeros((2, 3, BINS), dtype=torch.int64, device=dev),
               hist_grad=torch.zeros((2, BINS), dtype=torch.int64, device=dev))
    for i in range(0, heads['loc'].shape[0], batch):
        sl = slice(i, i + batch)
        ops.anchor_stats(heads['loc'][sl], heads['conf'][sl], heads['prop_conf'][sl], heads['center'][sl], heads['act'][sl],
                         heads['prop_act'][sl], priors, gt[sl], gvalid[sl], CLIP, OVERLAP, True, C, target, BINS, BINS, out=out,
                         rows=False)
    return out['hist_score'].cpu().numpy(), out['hist_grad'].cpu().numpy()


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--windows', type=int, default=3400)
    p.add_argument('--batch', type=int, default=128)
    p.add_argument('--target', type=str, default='half_au')
    p.add_argument('--runs', type=int, default=5)
    p.add_argument('--warmup', type=int, default=2)
    p.add_argument('--out', type=str, default=None)
    args = p.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("micro_anchor_stats.py measures on the GPU; none found")
    rs = np.random.RandomState(0)
    N = args.windows
    dev = torch.device('cuda', 0)
    f = lambda a: torch.from_numpy(a.astype(np.float32)).to(dev)
    heads = dict(loc=f(rs.uniform(2.0, 40.0, (N, K, 2))), conf=f(rs.normal(0.0, 2.0, (N, K, C))),
                 prop_conf=f(rs.normal(0.0, 2.0, (N, K, C))), center=f(rs.normal(0.0, 1.0, (N, K, 1))),
                 act=f(rs.normal(0.0, 1.0, (N, K, 1))), prop_act=f(rs.normal(0.0, 1.0, (N, K, 1))))
    priors = f(np.array([(c + 0.5) / t for t in LEVELS for c in range(t)]))
    start = rs.uniform(0.0, 0.7, (N, G))
    gt = f(np.stack([start, np.minimum(start + rs.uniform(0.05, 0.3, (N, G)), 1.0), rs.randint(1, C + 6, (N, G))], -1))
    gvalid = torch.from_numpy((np.arange(G)[None, :] < rs.randint(1, G + 1, (N, 1))).astype(np.uint8)).to(dev)
    sync = torch.cuda.synchronize
    times = dict(host=[], kernel=[])
    differ = None
    for it in range(args.warmup + args.runs):
        sync()
        t0 = time.perf_counter()
        hs_h, hg_h = host_pass(heads, priors, gt, gvalid, args.target)
        t1 = time.perf_counter()
        hs_k, hg_k = kernel_pass(heads, priors, gt, gvalid, args.target, args.batch)
        sync()
        t2 = time.perf_counter()
        differ = int(np.abs(hs_h - hs_k).sum() + np.abs(hg_h - hg_k).sum())
        if differ > 1e-4 * hs_k.sum():
            raise SystemExit(f"the two paths disagree in {differ} counts of {int(hs_k.sum())}")
        if it >= args.warmup:
            times['host'].append((t1 - t0) * 1e3)
            times['kernel'].append((t2 - t1) * 1e3)
    result = dict(windows=N, batch=args.batch, target=args.target, runs=args.runs, warmup=args.warmup,
                  anchors=int(hs_k.sum()) // 2, gradient_rows=[int(x) for x in hg_k.sum(-1)], counts_that_differ=differ,
                  median_ms={k: float(np.median(v)) for k, v in times.items()}, all_ms=times)
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(line + "\n")
    return result


if __name__ == '__main__':
    main()
