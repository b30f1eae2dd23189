"""GPU: the decision edges both fused detection losses (csrc/loss.hip) have branches for and that random floats never reach:
torch's half / half gradient split on min / max ties, `iou < thr` at equality, the inclusive clamp backward at exactly +-10,
the first minimum among equal ground-truth areas, inert padded target rows, top_m <= 0, and ties by index in the ranking of the
negatives (signed zeros included).  Inputs: tests/loss_cases.py edge_* -- dyadic rationals, so every decision's operands are exact
and identical in the kernel and in the reference; tests/test_loss_cases_cpu.py asserts that each case sits exactly on its edge."""
import numpy as np
import pytest
import torch

import loss_cases as LC

pytestmark = pytest.mark.gpu
KINDS = ("thumos", "anet")
EDL = dict(evidence='exp', loss_type='log', iou_aware=True, with_focal=False, alpha=0.25, gamma=2, with_ibm=True, ibm_start=10,
           momentum=0.99, num_bins=50)
ACT = dict(margin=1.0, weight=0)
ANET_EDL = dict(evidence='exp', loss_type='log', iou_aware=True, with_ibm=True, ibm_start=10, momentum=0.99, num_bins=50)
W = {"thumos": (1.0, 10.0, 1.0, 10.0, 1.0, 1.0, 1.0), "anet": (1.0, 0.7, 1.3, 0.9, 1.1, 0.6, 1.2)}
NAMES = ("loc", "conf", "prop_loc", "prop_conf", "center", "act", "prop_act")


def _module(kind):
    if kind == "thumos":
        from opental_amd.thumos14 import multisegment_loss as M
    else:
        from opental_amd.anet import multisegment_loss as M
    return M


def run(kind, heads, targets, priors, fused, weights=None, nostage=0, padded=None):
    """One call of the open-set criterion (cls_mode 0, IBM off, overlap 0.5): (terms float32 tensor (7,) on the CPU, gradients of
    sum weights[i] term_i).  padded = (gt (B, G, 3), valid (B, G)) replaces the ragged target list."""
    from opental_amd import _lib as L
    from opental_amd.common.input_pipeline import PaddedTargets
    M = _module(kind)
    dev = torch.device("cuda", 0)
    M.FUSED = fused
    L.set_option("OTAL_LOSS_NOSTAGE", nostage)
    try:
        C = LC.EDGE[kind]["C"]
        if kind == "thumos":
            crit = M.MultiSegmentLoss(C, 0.5, 1.0, cls_loss_type='edl', edl_config=EDL, os_head=True, act_config=ACT).to(dev)
        else:
            crit = M.MultiSegmentLoss(C, 0.5, 1.0, cls_loss_type='edl', edl_config=ANET_EDL, os_head=True).to(dev)
        crit.cls_loss.epoch = 0
        xs = {k: torch.from_numpy(heads[k].copy()).to(dev).requires_grad_(True) for k in NAMES}
        pri = torch.from_numpy(priors).to(dev)
        if padded is not None:
            tg = PaddedTargets(torch.from_numpy(padded[0]).to(dev), torch.from_numpy(padded[1]).to(dev))
        else:
            tg = [torch.from_numpy(t).to(dev) for t in targets]
        if kind == "thumos":
            terms = crit(dict(xs, priors=pri), tg)
        else:
            terms = crit([xs["loc"], xs["conf"], xs["prop_loc"], xs["prop_conf"], xs["center"], pri, xs["act"], xs["prop_act"]], tg)
        name = type(terms[0].grad_fn).__name__
        assert ('DetectionLossFunction' in name) == fused, name
        sum(w * t for w, t in zip(weights or W[kind], terms)).backward()
        grads = {k: (v.grad.detach().cpu() if v.grad is not None else torch.zeros(v.shape)) for k, v in xs.items()}
        return torch.stack([t.detach().reshape(()) for t in terms]).cpu(), grads
    finally:
        M.FUSED = True
        L.set_option("OTAL_LOSS_NOSTAGE", 0)


def close(kind, got, want):
    """The bounds of the fused-vs-torch pairing in tests/test_loss_gpu.py and tests/test_anet_gpu.py (2e-5)."""
    (t1, g1), (t0, g0) = got, want
    t1, t0 = t1.double().numpy(), t0.double().numpy()
    assert np.isfinite(t1).all()
    assert (np.abs(t1 - t0) <= 2e-5 * np.maximum(1.0, np.abs(t0)) if kind == "anet" else
            np.isclose(t1, t0, rtol=2e-5, atol=1e-6)).all(), (t1, t0)
    for k in g0:
        scale = max(float(g0[k].abs().max()), 1e-12)
        err = float((g1[k] - g0[k]).abs().max())
        assert err <= 2e-5 * scale + 1e-9, (k, err, scale, int((g1[k] - g0[k]).abs().argmax()))


@pytest.mark.parametrize("kind", KINDS)
def test_min_max_ties_split_the_gradient_in_halves(kind):
    """loc == loc_t (and a refined segment == loc_t): every min / max of the GIoU term and of the quality head's tIoU ties, and
    torch sends half of the gradient to each side (dmin_da / dmax_da).  With all four tied, tIoU = 1 is a stationary point of
    GIoU under that rule: the coarse-localisation gradient of those anchors is exactly 0, which no one-sided rule gives."""
    heads, targets, priors, info = LC.edge_ties(kind)
    close(kind, run(kind, heads, targets, priors, True), run(kind, heads, targets, priors, False))
    only_l = (1.0, 0, 0, 0, 0, 0, 0)
    _, g = run(kind, heads, targets, priors, True, weights=only_l)
    _, g0 = run(kind, heads, targets, priors, False, weights=only_l)
    assert float(g["loc"][0, info["full"]].abs().max()) == 0.0 == float(g0["loc"][0, info["full"]].abs().max())
    assert float(g["loc"][0, info["half"]].abs().min()) > 0.0          # one side tied: the other side still pulls
    close(kind, (torch.zeros(7), g), (torch.zeros(7), g0))


@pytest.mark.parametrize("kind", KINDS)
def test_iou_equal_to_the_threshold_stays_a_refined_positive(kind):
    """tIoU == 0.5 exactly is not `< 0.5`: anchor X is a positive of the refined stage, anchor Y (a few ulps below) is not --
    read off the refined-L1 gradient, which only refined positives receive."""
    heads, targets, priors, info = LC.edge_threshold(kind)
    close(kind, run(kind, heads, targets, priors, True), run(kind, heads, targets, priors, False))
    only_pl = (0, 0, 1.0, 0, 0, 0, 0)
    for fused in (True, False):
        t, g = run(kind, heads, targets, priors, fused, weights=only_pl)
        assert float(g["prop_loc"][0, info["x"]].abs().min()) > 0.0, fused
        assert float(g["prop_loc"][0, info["y"]].abs().max()) == 0.0, fused


@pytest.mark.parametrize("nostage", [0, 1])
@pytest.mark.parametrize("kind", KINDS)
def test_clamp_backward_is_inclusive_at_plus_minus_10(kind, nostage):
    """Logits at exactly +-10 carry gradient, one float beyond (and +-30) none -- in positive rows (classification term), in
    negative rows and in every row of prop_conf (IoU-calibration term), in the LDS-staged and in the unstaged THUMOS14 kernel."""
    heads, targets, priors, info = LC.edge_clamp(kind)
    got = run(kind, heads, targets, priors, True, nostage=nostage)
    close(kind, got, run(kind, heads, targets, priors, False))
    rows, is_pos = info["rows"], info["is_pos"]
    for name in ("conf", "prop_conf"):
        z = torch.from_numpy(heads[name][0, rows, :8])
        g = got[1][name][0, rows, :8]
        outside = z.abs() > 10
        assert int(outside.sum()) == 24 and int((z.abs() == 10).sum()) == 12
        assert float(g[outside].abs().max()) == 0.0, name
        carries = torch.from_numpy(is_pos)[:, None].expand(6, 8) if name == "conf" else torch.ones(6, 8, dtype=torch.bool)
        assert bool((g[~outside & carries] != 0).all()), (name, g)
        assert float(g[~carries].abs().max() if (~carries).any() else 0.0) == 0.0


@pytest.mark.parametrize("variant", ["equal_area", "equal_area_swapped", "duplicate"])
@pytest.mark.parametrize("kind", KINDS)
def test_first_of_equal_ground_truths_wins(kind, variant):
    """Two valid targets of equal area around an anchor (and the same segment twice with two labels): the first row's label is
    classified -- its logit is the only one of the row with a negative gradient (1 / S - 1 / alpha_y < 0)."""
    heads, targets, priors, info = LC.edge_ground_truths(kind, variant)
    got = run(kind, heads, targets, priors, True)
    close(kind, got, run(kind, heads, targets, priors, False))
    _, g = run(kind, heads, targets, priors, True, weights=(0, 1.0, 0, 0, 0, 0, 0))
    rows = g["conf"][0, info["both"]]
    assert len(info["both"]) > 0 and bool((rows[:, info["label"] - 1] < 0).all())
    assert int((rows < 0).sum()) == len(info["both"])


@pytest.mark.parametrize("kind", KINDS)
def test_padded_target_rows_are_inert(kind):
    """Rows with valid = 0 filled with finite garbage (segments that would win every anchor, labels out of range) and a larger G
    leave every bit of the terms and gradients as the zero-padded run has them."""
    heads, targets, priors, _ = LC.edge_ground_truths(kind, "equal_area")
    rows = targets[0]

    def padded(G, garbage):
        gt = np.zeros((1, G, 3), np.float32)
        valid = np.zeros((1, G), np.uint8)
        gt[0, :2], valid[0, :2] = rows, 1
        if garbage:
            gt[0, 2:] = [[0.0, 1.0, 11.0], [0.3, 0.31, 7.0], [-5.0, 9.0, 1e6], [0.25, 0.5, -3.0]][:G - 2]
        return gt, valid
    base = run(kind, heads, None, priors, True, padded=padded(3, False))
    ragged = run(kind, heads, targets, priors, True)
    for other in (ragged, run(kind, heads, None, priors, True, padded=padded(3, True)),
                  run(kind, heads, None, priors, True, padded=padded(6, True))):
        assert torch.equal(base[0], other[0]), (base[0], other[0])
        for k in base[1]:
            assert torch.equal(base[1][k], other[1][k]), k


def _pu_reference(kind, heads, info):
    """oracle.actionness_loss (stable sort of the negatives: ascending score, equal scores by index) + torch-CPU autograd on the
    sample's scores: per pass (term, gradient)."""
    from oracle import afsd_oracle as O
    res = []
    for name in ("act", "prop_act"):
        x = torch.from_numpy(heads[name][0].copy()).requires_grad_(True)
        loss, cnt = O.actionness_loss(x, torch.from_numpy(info["pos"].astype(np.float32)), 0.0 if kind == "thumos" else 0.1, 1.0)
        (loss / cnt).backward()
        res.append((float(loss.detach() / cnt), x.grad.clone(), cnt))
    return res


@pytest.mark.parametrize("variant", ["tie_straddle", "signed_zero", "all_equal", "npos1", "npos2"])
@pytest.mark.parametrize("kind", KINDS)
def test_negatives_rank_by_score_then_index(kind, variant):
    """The positive-unlabelled actionness terms when the top-m cut falls inside a group of equal scores, when all scores are equal,
    and when top_m is 0 (one positive: every negative is used) or 1 (two positives: the single lowest negative, the lower index
    of two tied ones).  -0.0 and +0.0 are EQUAL scores: the index decides, as in a stable sort."""
    heads, targets, priors, info = LC.edge_ranking(kind, variant)
    t, g = run(kind, heads, targets, priors, True, weights=(0, 0, 0, 0, 0, 1.0, 1.0))
    ref = _pu_reference(kind, heads, info)
    pos = torch.from_numpy(info["pos"])
    for p, name in enumerate(("act", "prop_act")):
        want, g_want, cnt = ref[p]
        expect = int(pos.sum()) + (info["top_m"] if info["top_m"] > 0 else int((~pos).sum()))
        assert int(cnt) == expect
        got_g = g[name][0].reshape(-1)
        g_want = g_want.reshape(-1)
        used, used_want = got_g != 0, g_want != 0
        used[info["top"]] = used_want[info["top"]] = False          # (ActivityNet: the hinge's arg max carries gradient, used or not)
        assert torch.equal(used, used_want), (name, torch.nonzero(used != used_want).reshape(-1).tolist())
        assert abs(float(t[5 + p]) - want) <= 2e-5 * max(1.0, abs(want)), (name, float(t[5 + p]), want)
        scale = float(g_want.abs().max())
        assert float((got_g - g_want).abs().max()) <= 2e-5 * scale + 1e-9, name
