"""The bits the fused detection losses give, case by case, for comparing two trees of this package (a refactor of the launch
path against its parent: every hash must be equal).

    python tools/loss_bits.py OUT.json [PACKAGE_ROOT]

PACKAGE_ROOT is the directory that holds the `opental_amd` to run (default: this repository); the seeded inputs come from
this repository's tests/*_common.py either way.  The loss is reached only through MultiSegmentLoss.forward and .backward(), so
the same file runs against any tree that has the two criteria.  Every case builds a fresh criterion and calls it twice on the
same leaves (the stateful variants update their EMA / populations in between); per call it records the SHA-256 of the float32
bytes of the terms, of every head's gradient and of the state tensor, and the name of the terms' autograd node.  The kernels
reduce in a fixed order without float atomics, so two runs of one tree give the same file; the hashes belong to one compiler
and one commit and are not kept."""
import hashlib
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 else REPO
sys.path[:0] = [ROOT, REPO, os.path.join(REPO, "tests")]

import numpy as np      # noqa: E402
import torch            # noqa: E402

import ablations_common as A            # noqa: E402
import anet_evidence_common as AE       # noqa: E402
import evidence_common as E             # noqa: E402

DEV = torch.device("cuda", 0)
FINAL = dict(A.BASE, **A.IBM)           # thumos14_opental_final.yaml
ANET_FINAL = dict(evidence='exp', loss_type='log', iou_aware=True, momentum=0.99, num_bins=50, **AE.IBM)    # anet_opental.yaml
RPL = dict(temperature=1, weight_pl=0.1)


def sha(t):
    return None if t is None else hashlib.sha256(t.detach().to(torch.float32).contiguous().cpu().numpy().tobytes()).hexdigest()


def thumos_targets(B):
    """Ragged lists: 3, 1, 2, 3, ... rows; the second sample's only segment holds no anchor centre (no positive)."""
    rs = np.random.RandomState(7)
    rows = lambda n: [[st, st + rs.uniform(0.05, 0.2), float(rs.randint(1, 16))] for st in rs.uniform(0.0, 0.8, n)]
    per_sample = [rows(3), [[0.2505, 0.2575, 3.0]]] + [rows(2 + i % 2) for i in range(B - 2)]
    return [torch.tensor(r, dtype=torch.float32, device=DEV) for r in per_sample[:B]]


def padded(targets, G):
    from opental_amd.common.input_pipeline import PaddedTargets
    gt = torch.zeros(len(targets), G, 3, device=DEV)
    valid = torch.zeros(len(targets), G, dtype=torch.uint8, device=DEV)
    for i, t in enumerate(targets):
        gt[i, :t.shape[0]], valid[i, :t.shape[0]] = t, 1
    return PaddedTargets(gt, valid)


def thumos_criterion(kind, os_head, cfg=None, epoch=10):
    from opental_amd.thumos14.multisegment_loss import MultiSegmentLoss
    key = dict(edl='edl_config', rpl='rpl_config').get(kind)
    crit = MultiSegmentLoss(15 if os_head else 16, 0.5, 1.0, cls_loss_type=kind, os_head=os_head, act_config=dict(A.ACT),
                            **({key: dict(cfg)} if key else {})).to(DEV)
    if kind == 'edl':
        crit.cls_loss.epoch = epoch
    return crit


def anet_criterion(kind, os_head, cfg=None):
    from opental_amd.anet.multisegment_loss import MultiSegmentLoss
    crit = MultiSegmentLoss(AE.classes(os_head), AE.PIOU, 1.0, cls_loss_type=kind, edl_config=None if cfg is None else dict(cfg),
                            os_head=os_head).to(DEV)
    if kind == 'edl':
        crit.cls_loss.epoch = AE.EPOCH
    return crit


def two_calls(crit, heads, weights, forward):
    """forward(leaves) -> the criterion's 7-tuple.  Two calls on fresh leaves of the same values."""
    calls = []
    for _ in range(2):
        leaves = {k: torch.from_numpy(v.copy()).to(DEV).requires_grad_(True) for k, v in heads.items()}
        terms = forward(leaves)
        n = 7 if crit.os_head else 5
        assert crit.os_head or (terms[5] is None and terms[6] is None)
        sum(w * t for w, t in zip(weights, terms[:n])).backward()
        state = crit.cls_loss.state() if hasattr(crit.cls_loss, 'state') else None
        calls.append(dict(terms=sha(torch.stack([t.detach() for t in terms[:n]])), grads={k: sha(v.grad) for k, v in leaves.items()},
                          state=sha(state), node=type(terms[1].grad_fn).__name__))
    return calls


def thumos_case(crit, B=2, targets=None, distances=False):
    C = crit.num_classes
    heads = E.head_outputs(100 + B, C, crit.os_head, B=B)
    if distances:                       # RPLHead's maps are distances to the class centres
        heads["conf"], heads["prop_conf"] = np.abs(heads["conf"]), np.abs(heads["prop_conf"])
    targets = thumos_targets(B) if targets is None else targets
    pri = A.priors(DEV)
    return two_calls(crit, heads, A.W, lambda x: crit(dict(x, priors=pri, act=x.get("act"), prop_act=x.get("prop_act")), targets))


def anet_case(crit, targets=None):
    heads = AE.head_outputs(11, crit.os_head)
    targets = AE.targets(dev=DEV) if targets is None else targets
    pri = AE.priors(DEV)
    return two_calls(crit, heads, AE.W, lambda x: crit([x["loc"], x["conf"], x["prop_loc"], x["prop_conf"], x["center"], pri,
                                                       x.get("act"), x.get("prop_act")], targets))


def main():
    from opental_amd import _lib as L
    import opental_amd
    assert os.path.dirname(os.path.dirname(os.path.abspath(opental_amd.__file__))) == ROOT, opental_amd.__file__
    out = {}
    # ---- THUMOS14: B = 2, K = 126, C = 15 (os_head) or 16
    out["final_e0"] = thumos_case(thumos_criterion('edl', True, FINAL, epoch=0))
    out["final_e10"] = thumos_case(thumos_criterion('edl', True, FINAL))
    out["final_e10_b1"] = thumos_case(thumos_criterion('edl', True, FINAL), B=1)
    out["final_e10_b14_unstaged"] = thumos_case(thumos_criterion('edl', True, FINAL), B=14)     # 14 * 126 * 15 floats > 96 KB
    out["final_e10_padded"] = thumos_case(thumos_criterion('edl', True, FINAL), targets=padded(thumos_targets(2), 5))
    L.set_option("OTAL_LOSS_NOSTAGE", 1)
    try:
        out["final_e10_nostage"] = thumos_case(thumos_criterion('edl', True, FINAL))
    finally:
        L.set_option("OTAL_LOSS_NOSTAGE", 0)
    out["focal_os_head"] = thumos_case(thumos_criterion('focal', True))
    out["closed_softmax"] = thumos_case(thumos_criterion('focal', False))
    out["closed_edl"] = thumos_case(thumos_criterion('edl', False, A.BASE))
    for name in A.VARIANTS:
        out["ablation_" + name] = thumos_case(A.criterion(name, DEV, epoch=10))
    for name in E.VARIANTS:
        out["evidence_" + name] = thumos_case(E.criterion(name, DEV, epoch=10))
    out["rpl"] = thumos_case(thumos_criterion('rpl', False, RPL), distances=True)
    out["gcpl"] = thumos_case(thumos_criterion('rpl', False, dict(RPL, gcpl=True)), distances=True)
    # ---- ActivityNet1.3: B = 2, K = 189, C = 150 (os_head) or 151
    out["anet_opental"] = anet_case(anet_criterion('edl', True, ANET_FINAL))
    out["anet_opental_padded"] = anet_case(anet_criterion('edl', True, ANET_FINAL), targets=padded(AE.targets(dev=DEV), 6))
    out["anet_closed_edl"] = anet_case(anet_criterion('edl', False, dict(evidence='exp', loss_type='log')))
    out["anet_closed_softmax"] = anet_case(anet_criterion('focal', False))
    for name in AE.VARIANTS:
        out["anet_" + name] = anet_case(AE.criterion(name, DEV))
    torch.cuda.synchronize()
    fused = [k for k, calls in out.items() if all('DetectionLossFunction' in c["node"] for c in calls)]
    assert len(fused) == len(out), sorted(set(out) - set(fused))       # every case is one the kernels cover
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(f"{len(out)} cases, 2 calls each -> {sys.argv[1]}")


if __name__ == "__main__":
    main()
