"""One (softplus, digamma) + IBM training step of the ActivityNet1.3 recipe (configs/anet_opental.yaml with that evidence and
loss type; 768-frame clips, the yaml's batch of 2, bf16, eager): the package's torch formulation of the loss
(anet.multisegment_loss.FUSED = False) next to the fused one (otal_detection_loss_anet_ev, csrc/loss.hip).

    python tools/micro_anet_evidence_loss.py [steps per block] [rounds]

One process, two trainers on the same seeded network and batch; after a warm-up of both, blocks of `steps` steps alternate
between the two (`rounds` blocks each), every step between two device events.  Reports the median, minimum and maximum step
time of each and the difference of the medians; asserts only that the fused criterion's terms come from
AnetDetectionLossFunction and the other one's do not.  Times are reported, not asserted.  Everything else of the step (network,
head tails with the softplus uncertainty item, optimiser) is the same code in both."""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
B = 2


def main():
    import numpy as np
    import torch
    import bench
    from opental_amd.anet import multisegment_loss as M
    from opental_amd.anet.train import build_training
    from opental_amd.common import config as C
    from opental_amd.common import ops
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 6
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    dev = torch.device("cuda", 0)
    ops.CONV_PRECISION = 1
    cfg = C.get_config([os.path.join(REPO, "configs", "anet_opental.yaml"), "--open_set", "--split", "0", "--lw", "1", "--cw", "1",
                        "--piou", "0.6", "--ssl", "0.1"])
    cfg['model']['evidence'] = 'softplus'
    cfg['training']['edl_config'].update(evidence='softplus', loss_type='digamma')
    clips, targets, scores = bench.synth_batch(B, 1000, dev, frames=768, classes=150, score_rows=3)
    trainers = {}
    for name in ("torch", "fused"):
        torch.manual_seed(5)
        _, crit, trainers[name] = build_training(cfg, dev, random_init=True)
        crit.cls_loss.epoch = 12            # past ibm_start: the IBM re-weighting runs inside the timed step
        assert crit.fused_route() == ('anet_ev', 0, (2, 1), True)
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
            pri = torch.tensor([[(c + 0.5) / t, l] for l, t in enumerate((96, 48, 24, 12, 6, 3)) for c in range(t)], device=dev)
            terms = tr.criterion([leaf(2, 189, 2, lo=2.0), leaf(2, 189, 150), leaf(2, 189, 2), leaf(2, 189, 150), leaf(2, 189, 1),
                                  pri, leaf(2, 189, 1), leaf(2, 189, 1)], targets[:2])
            assert ('AnetDetectionLossFunction' in type(terms[1].grad_fn).__name__) == (name == "fused"), name
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
        print(f"(softplus, digamma) ActivityNet training step, b = {B}, bf16, eager, {name:5s} loss: median "
              f"{res[name]['median_ms']:.2f} ms (min {res[name]['min_ms']:.2f}, max {res[name]['max_ms']:.2f}; {len(ms)} steps in "
              f"{rounds} alternating blocks)")
    print(f"difference of the medians: {res['torch']['median_ms'] - res['fused']['median_ms']:.2f} ms")
    print("ANET_EVIDENCE_STEP " + json.dumps(res))


if __name__ == "__main__":
    main()
