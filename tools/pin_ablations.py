"""tools/pin_ablations.py -- fixture generator for the THUMOS14 loss ablations (configs/ablations/thumos14_opental_{focal,ghm,ib,
hardmib,noMIB,noIoUC,noACT}.yaml of the reference: they differ from the final recipe in model.os_head and training.edl_config
only); runs where the reference source tree is available, never on the GPU machine.

Imports the reference through oracle.pin_against_reference.import_reference() and records, for every variant of VARIANTS, the
reference MultiSegmentLoss on B = 2 synthetic head outputs (K = 126; ragged ground truth, sample 1 without a positive anchor):
  * two consecutive calls at epoch 10 of ONE criterion (the GHM populations / the IBM EMA carry from the first to the second)
    and one call at epoch 0 of a fresh criterion (every gated rule inactive; focal has no gate);
  * per call the seven terms (five for noACT: no actionness heads), the autograd gradients of cost = sum_i W[i] * term_i with
    respect to every head output, and the state vector after the call (acc_sum for ghm, weight_accum for the IBM variants).
A variant without state gives the same call twice; the tool asserts that and records the second call's terms only.

The reference's own rows decide whether a fixture is usable: every row the reference hands to EvidenceLoss.edl_loss (both
passes) must keep g * num_bins at least 1e-3 away from an integer (ghm bins, the IBM ceil), the two largest alpha / S at
least 1e-3 apart (focal) and g * |z|_1 at least 1e-3 (ib).  The seed of the head outputs is searched until all hold, and the
margins are printed to the report.

Precision: each variant is run once more through the same reference code on float64 inputs; the report (and the fixture)
holds the largest relative difference of a term and the largest difference of a gradient relative to that gradient's
largest element -- the reference's own float32 error.  The tests of this kernel use 2e-5 for both; where four times the
reference's own error exceeds it (1 / (g |z|_1) of ib amplifies rounding), the tests allow four times that error instead,
read from the fixture (NAME_spread_terms, NAME_spread_grads).

Writes tests/golden/ablations.npz and tests/golden/PIN_REPORT_ablations.txt.

    python -m tools.pin_ablations
"""
import os
import sys

sys.dont_write_bytecode = True
os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
GOLD = os.path.join(REPO, "tests", "golden")

import numpy as np
import torch

from oracle import arch
from oracle.pin_against_reference import REF, import_reference, maxdiff

B = 2
W = (1.0, 10.0, 1.0, 10.0, 1.0, 1.0, 1.0)        # lw, cw, lw, cw, ctw, actw, actw of the THUMOS14 recipe
ACT = dict(margin=1.0, weight=0)
BASE = dict(evidence='exp', loss_type='log', iou_aware=True, with_focal=False, alpha=0.25, gamma=2)
IBM = dict(with_ibm=True, ibm_start=10, momentum=0.99, num_bins=50)
# name -> (os_head, edl_config): the seven yamls, and ghm once more with momentum 0 (the branch without the EMA)
VARIANTS = {
    "focal": (True, dict(BASE, with_focal=True)),
    "ghm": (True, dict(BASE, with_ghm=True, num_bins=30, momentum=0.85, ghm_start=10)),
    "ghm0": (True, dict(BASE, with_ghm=True, num_bins=30, momentum=0, ghm_start=10)),
    "ib": (True, dict(BASE, with_ibloss=True, ib_start=10)),
    "hardmib": (True, dict(BASE, **dict(IBM, momentum=0))),
    "noMIB": (True, dict(BASE)),
    "noIoUC": (True, dict(BASE, iou_aware=False, **IBM)),
    "noACT": (False, dict(BASE, **IBM)),
}
TARGETS = ([[0.10, 0.30, 3.0], [0.45, 0.62, 7.0], [0.70, 0.95, 15.0]],
           [[0.0, 0.005, 2.0]])             # no prior centre lies in [0, 0.005]: sample 1 has no positive anchor
MARGIN = 1e-3
LEAVES = ("loc", "conf", "prop_loc", "prop_conf", "center", "act", "prop_act")


def head_outputs(seed, C, os_head, B=B):
    """Synthetic (B, 126, .) head outputs: loc / prop_loc in the ranges the network produces, logits of a few units.
    Restated in tests/test_ablations_cpu.py."""
    rs = np.random.RandomState(seed)
    K = sum(arch.level_lengths())
    out = dict(loc=rs.uniform(2.0, 40.0, (B, K, 2)).astype(np.float32),
               conf=rs.normal(0.0, 2.0, (B, K, C)).astype(np.float32),
               prop_loc=rs.normal(0.0, 0.3, (B, K, 2)).astype(np.float32),
               prop_conf=rs.normal(0.0, 2.0, (B, K, C)).astype(np.float32),
               center=rs.normal(0.0, 1.0, (B, K, 1)).astype(np.float32))
    if os_head:
        out["act"] = rs.normal(0.0, 1.0, (B, K, 1)).astype(np.float32)
        out["prop_act"] = rs.normal(0.0, 1.0, (B, K, 1)).astype(np.float32)
    return out


def priors():
    return torch.tensor([[(c + 0.5) / t] for t in arch.level_lengths() for c in range(t)], dtype=torch.float32)


def state_of(cl):
    if getattr(cl, "with_ghm", False):
        return np.array(getattr(cl, "acc_sum", [0.0] * cl.num_bins), np.float64)
    if getattr(cl, "with_ibm", False):
        return cl.weight_accum.detach().double().numpy().copy()
    return np.zeros(0, np.float64)


def run(MultiSegmentLoss, name, heads, epoch, calls, dtype=torch.float32, rows=None):
    """`calls` consecutive calls of one reference criterion; [(terms, grads, state)].  rows: a list that receives what the
    reference hands to edl_loss, (alpha, target, feat_norm) per pass."""
    os_head, cfg = VARIANTS[name]
    crit = MultiSegmentLoss(15 if os_head else 16, 0.5, 1.0, cls_loss_type='edl', edl_config=dict(cfg), os_head=os_head,
                            act_config=dict(ACT))
    crit.cls_loss.epoch = epoch
    if rows is not None:
        inner = crit.cls_loss.edl_loss

        def spy(y, alpha, func=torch.log, target=None, feat_norm=None):
            rows.append((alpha.detach().clone(), target.detach().clone().view(-1), y.detach().clone(),
                         None if feat_norm is None else feat_norm.detach().clone()))
            return inner(y, alpha, func=func, target=target, feat_norm=feat_norm)
        crit.cls_loss.edl_loss = spy
    res = []
    for _ in range(calls):
        ins = {k: torch.from_numpy(v.copy()).to(dtype).requires_grad_(True) for k, v in heads.items()}
        out = dict(ins, priors=priors().to(dtype))
        out.setdefault("act", None); out.setdefault("prop_act", None)
        terms = crit(out, [torch.tensor(t, dtype=dtype) for t in TARGETS])
        n = 7 if os_head else 5
        assert os_head or (terms[5] is None and terms[6] is None)
        sum(w * t for w, t in zip(W, terms[:n])).backward()
        res.append((np.array([float(t) for t in terms[:n]], np.float64),
                    {k: v.grad.detach().double().numpy().copy() for k, v in ins.items()}, state_of(crit.cls_loss)))
    return res


def margins(name, rows):
    """The three margins over every row the reference classified (both passes); None where a margin does not apply."""
    _, cfg = VARIANTS[name]
    nb = cfg.get("num_bins", 50)
    edge, top2, ghat, n = None, None, None, 0
    for alpha, target, y, feat_norm in rows:
        if alpha.shape[0] == 0:
            continue
        n += alpha.shape[0]
        S = alpha.sum(1, keepdim=True)
        g = (torch.abs(1 / alpha - alpha.shape[1] / S) * y).sum(1).double()
        if cfg.get("with_ghm") or cfg.get("with_ibm"):
            x = g * nb
            d = float((x - torch.round(x)).abs().min())
            edge = d if edge is None else min(edge, d)
        if cfg.get("with_focal"):
            p = torch.sort(alpha / S, dim=1, descending=True)[0]
            d = float((p[:, 0] - p[:, 1]).min())
            top2 = d if top2 is None else min(top2, d)
        if cfg.get("with_ibloss"):
            d = float((g * feat_norm.double()).min())
            ghat = d if ghat is None else min(ghat, d)
    return edge, top2, ghat, n


def spread(a32, a64):
    """Largest relative term difference and largest gradient difference relative to the gradient's largest element."""
    t = max(abs(x - y) / max(abs(y), 1e-30) for (t32, _, _), (t64, _, _) in zip(a32, a64) for x, y in zip(t32, t64))
    g = max(float(np.abs(g32[k] - g64[k]).max()) / max(float(np.abs(g64[k]).max()), 1e-30)
            for (_, g32, _), (_, g64, _) in zip(a32, a64) for k in g32)
    return t, g


def check_against_package(name, heads, res, report):
    """The package's torch formulation on the host, against what was just recorded."""
    from opental_amd.thumos14.multisegment_loss import MultiSegmentLoss
    os_head, cfg = VARIANTS[name]
    crit = MultiSegmentLoss(15 if os_head else 16, 0.5, 1.0, cls_loss_type='edl', edl_config=dict(cfg), os_head=os_head,
                            act_config=dict(ACT))
    crit.cls_loss.epoch = 10
    worst_t = worst_g = 0.0
    for call in (1, 2):
        ins = {k: torch.from_numpy(v.copy()).requires_grad_(True) for k, v in heads.items()}
        out = dict(ins, priors=priors())
        out.setdefault("act", None); out.setdefault("prop_act", None)
        terms = crit(out, [torch.tensor(t) for t in TARGETS])
        n = 7 if os_head else 5
        sum(w * t for w, t in zip(W, terms[:n])).backward()
        want = res[f"{name}_call{call}_terms"]
        worst_t = max(worst_t, max(abs(float(t) - r) / max(abs(r), 1e-30) for t, r in zip(terms[:n], want)))
        if f"{name}_call{call}_grad_loc" in res:
            worst_g = max(worst_g, max(maxdiff(v.grad, torch.from_numpy(res[f"{name}_call{call}_grad_{k}"]))
                                       / max(float(np.abs(res[f"{name}_call{call}_grad_{k}"]).max()), 1e-30)
                                       for k, v in ins.items()))
    report.append(f"{name}: package torch formulation vs reference: max rel term diff {worst_t:.3e}, max grad diff / scale {worst_g:.3e}")


def main():
    torch.manual_seed(0)
    _, MultiSegmentLoss, _, _, _ = import_reference()
    report = ["loss-ablation fixtures (tools/pin_ablations.py): reference MultiSegmentLoss + EvidenceLoss, B = 2, K = 126",
              f"margins required on every row the reference classified (both passes): >= {MARGIN:g}"]
    seed = None
    for cand in range(31, 200):
        ok = True
        for name, (os_head, _) in VARIANTS.items():
            rows = []
            run(MultiSegmentLoss, name, head_outputs(cand, 15 if os_head else 16, os_head), 10, 1, rows=rows)
            if any(m is not None and m < MARGIN for m in margins(name, rows)[:3]):
                ok = False
                break
        if ok:
            seed = cand
            break
    assert seed is not None, "no seed meets the margins"
    res = {"targets_" + str(i): np.array(t, np.float32) for i, t in enumerate(TARGETS)}
    res["weights"] = np.array(W, np.float64)
    res["seed"] = np.array(seed)
    report.append(f"head-output seed {seed} (searched from 31)")
    for name, (os_head, cfg) in VARIANTS.items():
        heads = head_outputs(seed, 15 if os_head else 16, os_head)
        rows = []
        two = run(MultiSegmentLoss, name, heads, 10, 2, rows=rows)
        edge, top2, ghat, n = margins(name, rows)
        fmt = lambda v: "n/a" if v is None else f"{v:.4g}"
        report.append(f"{name}: {n} classified rows over 2 calls x 2 passes; min |g * num_bins - integer| {fmt(edge)}, "
                      f"min top-2 gap of alpha / S {fmt(top2)}, min g * |z|_1 {fmt(ghat)}")
        assert all(m is None or m >= MARGIN for m in (edge, top2, ghat)), (name, edge, top2, ghat)
        zero = run(MultiSegmentLoss, name, heads, 0, 1)
        stateful = two[0][2].size > 0 and not (cfg.get("with_ghm") and cfg["momentum"] == 0)
        for tag, (terms, grads, state) in (("call1", two[0]), ("call2", two[1]), ("epoch0", zero[0])):
            res[f"{name}_{tag}_terms"] = terms
            res[f"{name}_{tag}_state"] = state
            if tag == "call2" and not stateful:
                assert np.array_equal(terms, two[0][0]) and all(np.array_equal(grads[k], two[0][1][k]) for k in grads), name
                continue                    # the same call twice: the first call's gradients stand for both
            for k, v in grads.items():
                res[f"{name}_{tag}_grad_{k}"] = v.astype(np.float32)
        report.append(f"{name}: terms call 1 {', '.join(f'{t:.6f}' for t in two[0][0])}")
        report.append(f"{name}: terms call 2 {', '.join(f'{t:.6f}' for t in two[1][0])}"
                      + ("" if stateful else "  (no state: identical to call 1, gradients not stored twice)"))
        report.append(f"{name}: terms epoch 0 {', '.join(f'{t:.6f}' for t in zero[0][0])}")
        t64 = run(MultiSegmentLoss, name, heads, 10, 2, dtype=torch.float64)
        st, sg = spread(two, t64)
        res[f"{name}_spread_terms"] = np.array(st)
        res[f"{name}_spread_grads"] = np.array(sg)
        wider = 4 * st > 2e-5 or 4 * sg > 2e-5
        report.append(f"{name}: reference float32 vs the same code on float64 inputs: max rel term diff {st:.3e}, "
                      f"max grad diff / scale {sg:.3e}; the tests allow max(2e-5, 4 x that): "
                      + (f"terms rtol {max(2e-5, 4 * st):.3e}, gradients {max(2e-5, 4 * sg):.3e} of the scale" if wider
                         else "2e-5 stands for both"))
        check_against_package(name, heads, res, report)
    path = os.path.join(GOLD, "ablations.npz")
    np.savez_compressed(path, **res)
    size = os.path.getsize(path)
    report.append(f"tests/golden/ablations.npz: {size} bytes")
    assert size < 600 * 1024, size
    with open(os.path.join(GOLD, "PIN_REPORT_ablations.txt"), "w") as f:
        f.write("\n".join(report) + "\n")
    print("\n".join(report))
    leftovers = [os.path.join(d_, n) for d_, _, fs in os.walk(REF) for n in fs if n.endswith(".pyc")]
    assert not leftovers, leftovers


if __name__ == "__main__":
    main()
