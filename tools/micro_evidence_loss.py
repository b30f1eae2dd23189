"""One (softplus, digamma) training step of the THUMOS14 recipe at b = 8, bf16, eager: the package's torch formulation of the
loss (multisegment_loss.FUSED = False) next to the single-launch loss (otal_detection_loss_ev, csrc/loss.hip).

    python tools/micro_evidence_loss.py [steps per block] [rounds]

One process, two trainers on the same seeded network and batch; after a warm-up of both, blocks of `steps` steps alternate
between the two (`rounds` blocks each), every step between two device events.  Reports the median, minimum and maximum step
time of each and the difference of the medians; asserts only that the fused criterion's terms come from DetectionLossFunction
and the other one's do not.  Times are reported, not asserted.  Everything else of the step (network, head tails with the
softplus uncertainty item, optimiser) is the same code in both."""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
B = 8
EDL = dict(evidence='softplus', loss_type='digamma', iou_aware=True, with_focal=False, alpha=0.25, gamma=2,
           with_ibm=True, ibm_start=0, momentum=0.99, num_bins=50)


def main():
    import numpy as np
    import torch
    import bench
    from opental_amd.common import ops
    from opental_amd.thumos14 import multisegment_loss as M
    from opental_amd.thumos14.BDNet import BDNet, DEFAULT_MODEL_CFG
    from opental_amd.thumos14.train import DetectorTrainer
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 6
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    dev = torch.device("cuda", 0)
    ops.CONV_PRECISION = 1
    clips, targets, scores = bench.synth_batch(B, 1000, dev)
    W = dict(lw=1.0, cw=10.0, ctw=1.0, actw=1.0, ssl=0.001)
    trainers = {}
    for name in ("torch", "fused"):
        torch.manual_seed(5)
        net = BDNet(in_channels=3, training=False, use_edl=True, cfg=dict(DEFAULT_MODEL_CFG, os_head=True, evidence='softplus'))
        net.backbone._model.apply(BDNet.weight_init)
        crit = M.MultiSegmentLoss(15, 0.5, 1.0, cls_loss_type='edl', edl_config=dict(EDL), os_head=True,
                                  act_config=dict(margin=1.0, weight=0)).to(dev)
        trainers[name] = DetectorTrainer(net.to(dev).train(), crit, W, lr=1e-5, weight_decay=1e-3)
    times = {name: [] for name in trainers}

    def block(name, n, record):
        M.FUSED = name == "fused"
        try:
            tr = trainers[name]
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(n + 1)]
            ev[0].record()
            for i in range(n):
                cost = tr.step(clips, targets, scores)[0]
                ev[i + 1].record()
            torch.cuda.synchronize()
            assert np.isfinite(float(cost)), name
            if record:
                times[name] += [ev[i].elapsed_time(ev[i + 1]) for i in range(n)]
        finally:
            M.FUSED = True

    for name, tr in trainers.items():       # which formulation each criterion runs
        M.FUSED = name == "fused"
        try:
            g = torch.Generator().manual_seed(1)
            leaf = lambda *shape, lo=0.0: (lo + torch.rand(*shape, generator=g)).to(dev).requires_grad_(True)
            out = dict(loc=leaf(2, 126, 2, lo=2.0), conf=leaf(2, 126, 15), prop_loc=leaf(2, 126, 2), prop_conf=leaf(2, 126, 15),
                       center=leaf(2, 126, 1), act=leaf(2, 126, 1), prop_act=leaf(2, 126, 1),
                       priors=torch.tensor([[(c + 0.5) / t] for t in (64, 32, 16, 8, 4, 2) for c in range(t)], device=dev))
            terms = tr.criterion(out, targets[:2])
            assert ('DetectionLossFunction' in type(terms[1].grad_fn).__name__) == (name == "fused"), name
        finally:
            M.FUSED = True
    for name in trainers:
        block(name, 3, False)
    for _ in range(rounds):
        for name in trainers:
            block(name, steps, True)
    res = {}
    for name, ms in times.items():
        ms = sorted(ms)
        res[name] = dict(median_ms=ms[len(ms) // 2], min_ms=ms[0], max_ms=ms[-1], steps=len(ms))
        print(f"(softplus, digamma) training step, b = {B}, bf16, eager, {name:5s} loss: median {res[name]['median_ms']:.2f} ms "
              f"(min {res[name]['min_ms']:.2f}, max {res[name]['max_ms']:.2f}; {len(ms)} steps in {rounds} alternating blocks)")
    print(f"difference of the medians: {res['torch']['median_ms'] - res['fused']['median_ms']:.2f} ms")
    print("EVIDENCE_STEP " + json.dumps(res))


if __name__ == "__main__":
    main()
