"""Kernel-only times of the RPL / GCPL distance head (csrc/rplhead.hip), forward and backward, at B = 8, N = 126, C = 16,
D = 512, next to the reference's torch formulation (expanded form through rocBLAS) on the same device; and one RPL training
step next to the Softmax baseline's.

    python tools/micro_rpl.py [repeats]

The parent never touches the GPU: every measurement is a fresh child process -- the two head workloads under
`rocprofv3 --kernel-trace --stats`, the training steps plain (wall clock between device events).  From the kernel trace it
ASSERTS the launch counts the head was designed for: one launch per forward, at most two per backward.  Times are reported,
not asserted."""
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
B, N, C, D = 8, 126, 16, 512


def _inputs(dev):
    import torch
    g = torch.Generator().manual_seed(0)
    x = torch.relu(torch.randn(B, D, N, generator=g)).to(dev).requires_grad_(True)
    cen = (0.1 * torch.randn(C, D, generator=g)).to(dev).requires_grad_(True)
    gy = torch.randn(B, C, N, generator=g).to(dev)
    return x, cen, gy


def child_head(kind, reps):
    import torch
    from opental_amd.common import ops
    dev = torch.device("cuda", 0)
    x, cen, gy = _inputs(dev)

    def torch_form(x, cen):         # AFSD/common/layers.py:327-351
        f = x.permute(0, 2, 1).contiguous().view(-1, D)
        f2 = torch.sum(torch.pow(f, 2), dim=1, keepdim=True)
        c2 = torch.sum(torch.pow(cen, 2), dim=1, keepdim=True)
        d = (f2 - 2 * torch.matmul(f, torch.transpose(cen, 1, 0)) + torch.transpose(c2, 1, 0)) / float(D)
        return d.view(-1, N, C).permute(0, 2, 1).contiguous()
    fn = (lambda: ops.RPLHeadFunction.apply(x, cen)) if kind == "hip" else (lambda: torch_form(x, cen))
    for _ in range(reps):
        x.grad = cen.grad = None
        fn().backward(gy)
    torch.cuda.synchronize()


def child_steps(steps):
    import numpy as np
    import torch
    import bench
    from opental_amd.common import ops
    from opental_amd.thumos14.BDNet import BDNet, DEFAULT_MODEL_CFG
    from opental_amd.thumos14.multisegment_loss import MultiSegmentLoss
    from opental_amd.thumos14.train import DetectorTrainer
    dev = torch.device("cuda", 0)
    ops.CONV_PRECISION = 1
    clips, targets, scores = bench.synth_batch(B, 1000, dev)
    W = dict(lw=1.0, cw=10.0, ctw=1.0, actw=1.0, ssl=0.001)
    out = {}
    for name in ("softmax", "rpl", "gcpl"):
        torch.manual_seed(5)
        net = BDNet(in_channels=3, training=False, use_rpl=name != "softmax", cfg=dict(DEFAULT_MODEL_CFG, os_head=False))
        net.backbone._model.apply(BDNet.weight_init)
        net = net.to(dev).train()
        if name == "softmax":
            crit = MultiSegmentLoss(16, 0.5, 1.0, cls_loss_type='focal')
        else:
            crit = MultiSegmentLoss(16, 0.5, 1.0, cls_loss_type='rpl',
                                    rpl_config=dict(temperature=1, weight_pl=0.1, gcpl=name == "gcpl"))
        tr = DetectorTrainer(net, crit.to(dev), W, lr=1e-5, weight_decay=1e-3)
        for _ in range(3):
            tr.step(clips, targets, scores)
        torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
        ev[0].record()
        for i in range(steps):
            cost = tr.step(clips, targets, scores)[0]
            ev[i + 1].record()
        torch.cuda.synchronize()
        ms = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(steps))
        assert np.isfinite(float(cost))
        out[name] = dict(median_ms=ms[len(ms) // 2], min_ms=ms[0], max_ms=ms[-1])
        del tr, net
    print("STEPS " + json.dumps(out))


def profiled(kind, reps):
    """Run child_head(kind) under the kernel trace; {kernel name: (calls, total ns)}."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "p", "--",
               sys.executable, os.path.abspath(__file__), "--child-head", kind, str(reps)]
        subprocess.run(cmd, check=True, timeout=240, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, cwd=d)
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        assert files, "no kernel_stats.csv from the kernel trace"
        return {r["Name"]: (int(r["Calls"]), float(r["TotalDurationNs"])) for r in csv.DictReader(open(files[0]))}


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    hip = profiled("hip", reps)
    head = {k: v for k, v in hip.items() if "rpl_head" in k}
    count = lambda pat: sum(v[0] for k, v in head.items() if pat in k)
    us = lambda pat: sum(v[1] for k, v in head.items() if pat in k) / 1e3 / reps
    n_fwd, n_dx, n_dc = count("rpl_head_fwd_kernel"), count("rpl_head_dx_kernel"), count("rpl_head_dcenters_kernel")
    print(f"distance head, B {B} N {N} C {C} D {D}, {reps} repeats")
    print(f"  HIP   forward {us('rpl_head_fwd_kernel'):7.1f} us in {n_fwd / reps:.0f} launch; backward "
          f"{us('rpl_head_dx_kernel') + us('rpl_head_dcenters_kernel'):7.1f} us in {(n_dx + n_dc) / reps:.0f} launches "
          f"(dx {us('rpl_head_dx_kernel'):.1f}, dcenters {us('rpl_head_dcenters_kernel'):.1f})")
    assert n_fwd == reps, f"the head forward is one launch: {n_fwd} launches in {reps} forwards"
    assert n_dx + n_dc <= 2 * reps and n_dx + n_dc == count("rpl_head_") - n_fwd, \
        f"the head backward is at most two launches: {n_dx + n_dc} launches in {reps} backwards"
    tor = profiled("torch", reps)
    rep = {k: v for k, v in tor.items() if v[0] >= reps}       # what every repeat launches (not the one-off set-up)
    print(f"  torch forward + backward {sum(v[1] for v in rep.values()) / 1e3 / reps:7.1f} us in "
          f"{sum(v[0] for v in rep.values()) / reps:.0f} launches (expanded form, rocBLAS matmul)")
    own = {k: v for k, v in hip.items() if v[0] >= reps}
    print(f"  HIP   forward + backward {sum(v[1] for v in own.values()) / 1e3 / reps:7.1f} us in "
          f"{sum(v[0] for v in own.values()) / reps:.0f} launches (with autograd's own launches)")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-steps", "12"], check=True, timeout=420,
                       capture_output=True, text=True)
    steps = json.loads(next(l for l in r.stdout.splitlines() if l.startswith("STEPS "))[6:])
    for name, v in steps.items():
        print(f"  training step b = {B}, bf16, eager: {name:8s} median {v['median_ms']:.2f} ms (min {v['min_ms']:.2f}, max {v['max_ms']:.2f})")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child-head":
        child_head(sys.argv[2], int(sys.argv[3]))
    elif len(sys.argv) > 1 and sys.argv[1] == "--child-steps":
        child_steps(int(sys.argv[2]))
    else:
        main()
