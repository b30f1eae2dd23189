"""tools/pin_anet_evidence.py -- fixture generator for the EDL settings of the ActivityNet1.3 recipe beyond its shipped configs:
training.edl_config.evidence relu | softplus, loss_type digamma | mse, and the influence-balanced weight over the closed set
(AFSD/anet/cls_loss.py:79-246, anet/multisegment_loss.py:87-301); runs where the reference source tree is available, never on
the GPU machine, in a process of its own.

Imports the reference's AFSD.anet.multisegment_loss on the CPU (configs/anet_edl.yaml in sys.argv for its config module; the
criterion takes num_classes / os_head / edl_config as constructor arguments) and records, on the synthetic head outputs of
tests/anet_evidence_common.py (B = 2, K = 189: the recipe's priors with level ids; C = 150 with os_head, 151 closed set; ragged
targets, sample 1 without a positive anchor; logits kept 1e-3 off the decision edges 0, 20 and +-10), for every variant of
anet_evidence_common.VARIANTS -- the eight non-default (evidence, loss_type) pairs with os_head (log / digamma with IBM at an
epoch >= ibm_start, mse without), and closed set (exp, log) with IBM, (softplus, digamma) with IBM, (relu, mse), (relu, log)
with iou_aware:
  * the seven terms (five, closed set) of one call at epoch 12;
  * the autograd gradients of cost = sum_i W[i] term_i with respect to conf and prop_conf at strided() probe positions.  The
    gradients of the other heads do not depend on the evidence function or the loss type: the tool asserts that they equal those
    of the (exp, log) criterion bit for bit and stores them once per head layout (base_os_grad_*, base_closed_grad_*);
  * NAME_spread_terms / NAME_spread_grads: the reference's own float32 error against the same code on float64 inputs.
Every stored value is asserted finite, no row of logits is all <= 0 (relu: u = 1 gives log(1 - u) = -inf, in the reference too),
and the head-output seed is searched until both hold.

Writes tests/golden/anet_evidence.npz and tests/golden/PIN_REPORT_anet_evidence.txt.

    python -m tools.pin_anet_evidence
"""
import os
import sys

sys.dont_write_bytecode = True
os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
GOLD = os.path.join(REPO, "tests", "golden")

import numpy as np
import torch

import anet_evidence_common as AE
import evidence_common as E
from oracle.pin_against_reference import REF
from tools.pin_ablations import spread

LIMIT = 472 * 1024          # the largest fixture present (ablations.npz)


def import_reference():
    sys.path.insert(0, REF)
    sys.argv = ["pin", os.path.join(REF, "configs/anet_edl.yaml"), "--open_set", "--split", "0", "--lw", "1", "--cw", "1",
                "--piou", str(AE.PIOU)]
    torch.Tensor.cuda = lambda self, *a, **k: self
    import AFSD.anet.multisegment_loss as ref_loss
    from AFSD.common.config import config
    assert config['dataset']['training']['clip_length'] == 768
    return ref_loss


def run(ref_loss, cfg, os_head, heads, dtype=torch.float32):
    """One call at epoch AE.EPOCH of a reference criterion: [(terms, grads of every head, None)] (the shape spread() reads)."""
    ref_loss.prior_lb = ref_loss.prior_rb = None            # module globals cached from the first priors seen (dtype!)
    crit = ref_loss.MultiSegmentLoss(AE.classes(os_head), AE.PIOU, 1.0, cls_loss_type='edl', edl_config=dict(cfg), os_head=os_head)
    crit.cls_loss.epoch = AE.EPOCH
    ins = {k: torch.from_numpy(v.copy()).to(dtype).requires_grad_(True) for k, v in heads.items()}
    pred = [ins["loc"], ins["conf"], ins["prop_loc"], ins["prop_conf"], ins["center"], AE.priors().to(dtype), ins.get("act"),
            ins.get("prop_act")]
    terms = crit(pred, [torch.tensor(t, dtype=dtype) for t in AE.TARGETS])
    n = 7 if os_head else 5
    assert os_head or (terms[5] is None and terms[6] is None)
    sum(w * t for w, t in zip(AE.W, terms[:n])).backward()
    return [(np.array([float(t) for t in terms[:n]], np.float64),
             {k: v.grad.detach().double().numpy().copy() for k, v in ins.items()}, None)]


def finite(res):
    return all(np.isfinite(t).all() and all(np.isfinite(g).all() for g in gr.values()) for t, gr, _ in res)


def usable(ref_loss, seed):
    """No row of logits all <= 0, every reference value of every variant finite at this head-output seed."""
    for os_head in (True, False):
        h = AE.head_outputs(seed, os_head)
        if any((h[k] <= 0).all(-1).any() for k in AE.GRAD_KEYS):
            return False
    return all(finite(run(ref_loss, cfg, os_head, AE.head_outputs(seed, os_head))) for os_head, cfg in AE.VARIANTS.values())


def check_against_package(name, heads, res, report):
    """The package's torch formulation on the host, against what was just recorded."""
    got = AE.call(AE.criterion(name), heads, AE.targets())
    assert 'AnetDetectionLossFunction' not in got[2]
    d = float(np.abs(got[0] - res[f"{name}_terms"]).max())
    g = max(float(np.abs(AE.strided(got[1][k]) - res[f"{name}_grad_{k}"]).max()) for k in AE.GRAD_KEYS)
    report.append(f"{name}: package torch formulation vs reference: max |term diff| {d:.3e}, max |grad diff| at the probes {g:.3e}")


def main():
    torch.manual_seed(0)
    ref_loss = import_reference()
    report = ["ActivityNet1.3 evidence / loss-type fixtures (tools/pin_anet_evidence.py): reference AFSD.anet MultiSegmentLoss + "
              f"EvidenceLoss on the CPU; B = {AE.B}, K = 189, epoch {AE.EPOCH}"]
    seed = next((s for s in range(71, 200) if usable(ref_loss, s)), None)
    assert seed is not None, "no seed meets the conditions"
    report.append(f"head-output seed {seed} (searched from 71): no row of logits all <= 0, every reference value finite")
    res = {"targets_" + str(i): np.array(t, np.float32) for i, t in enumerate(AE.TARGETS)}
    res["weights"] = np.array(AE.W, np.float64)
    res["seed"] = np.array(seed)
    res["epoch"] = np.array(AE.EPOCH)
    base = {}
    for os_head, tag in ((True, "base_os"), (False, "base_closed")):
        heads = AE.head_outputs(seed, os_head)
        for k in AE.GRAD_KEYS:
            assert min(float(np.abs(heads[k] - e).min()) for e in E.EDGES) >= E.EDGE_MARGIN
            assert not (heads[k] <= 0).all(-1).any()
        base[os_head] = run(ref_loss, dict(evidence='exp', loss_type='log'), os_head, heads)[0][1]
        for k, v in base[os_head].items():
            if k not in AE.GRAD_KEYS:
                assert np.isfinite(v).all()
                res[f"{tag}_grad_{k}"] = v.astype(np.float32)
    for name, (os_head, cfg) in AE.VARIANTS.items():
        heads = AE.head_outputs(seed, os_head)
        one = run(ref_loss, cfg, os_head, heads)
        assert finite(one), name
        terms, grads, _ = one[0]
        res[f"{name}_terms"] = terms
        for k, v in grads.items():
            if k in AE.GRAD_KEYS:
                res[f"{name}_grad_{k}"] = AE.strided(v).astype(np.float32)
                assert float(np.abs(res[f"{name}_grad_{k}"]).max()) > 0, (name, k)
            else:                               # loc / prop_loc / center / act / prop_act: as with (exp, log)
                assert np.array_equal(v, base[os_head][k]), (name, k)
        st, sg = spread(one, run(ref_loss, cfg, os_head, heads, dtype=torch.float64))
        res[f"{name}_spread_terms"] = np.array(st)
        res[f"{name}_spread_grads"] = np.array(sg)
        report.append(f"{name}: terms {', '.join(f'{t:.6f}' for t in terms)}")
        report.append(f"{name}: reference float32 vs the same code on float64 inputs: max rel term diff {st:.3e}, max grad diff / "
                      f"scale {sg:.3e}; the tests allow terms rtol {max(2e-5, 4 * st):.3e}, gradients {max(2e-5, 4 * sg):.3e} of "
                      "the scale")
        check_against_package(name, heads, res, report)
    assert all(np.isfinite(v).all() for v in res.values())
    path = os.path.join(GOLD, "anet_evidence.npz")
    np.savez_compressed(path, **res)
    size = os.path.getsize(path)
    report.append(f"tests/golden/anet_evidence.npz: {size} bytes")
    assert size <= LIMIT, size
    with open(os.path.join(GOLD, "PIN_REPORT_anet_evidence.txt"), "w") as f:
        f.write("\n".join(report) + "\n")
    print("\n".join(report))
    leftovers = [os.path.join(d_, n) for d_, _, fs in os.walk(REF) for n in fs if n.endswith(".pyc")]
    assert not leftovers, leftovers


if __name__ == "__main__":
    main()
