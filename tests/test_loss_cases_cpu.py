"""CPU: every case of tests/loss_cases.py under the reference alone (oracle.afsd_oracle), so that the GPU comparisons of
tests/test_loss_sweeps_gpu.py and tests/test_anet_loss_sweeps_gpu.py cannot pass or fail because the REFERENCE sits on a decision:
positives in both stages and on both sides of anchor 1024, a top-m cut inside the negatives with a score gap, no positive within
1e-4 of a histogram bin edge, no tIoU within 1e-5 of the overlap threshold.  The cases of tests/test_loss_edges_gpu.py sit on such
edges on purpose: for them the exact condition is asserted instead."""
import numpy as np
import pytest
import torch

import loss_cases as LC
from oracle import afsd_oracle as O, arch

BIN_COUNTS = (50, 30)       # the IBM EMA's bins and the GHM ablation's


def _t(heads, targets, priors):
    out = {k: torch.from_numpy(v) for k, v in heads.items()}
    out["priors"] = torch.from_numpy(priors)
    return out, [torch.from_numpy(t) for t in targets]


def bin_margin(logits, y, rows, num_bins):
    """Smallest distance of gnorm * num_bins to an integer over `rows` (EvidenceLoss: gnorm = |1 / alpha_y - C / S|)."""
    z = logits.reshape(-1, logits.shape[-1]).astype(np.float64)[rows]
    al = np.exp(np.clip(z, -10, 10)) + 1
    g = np.abs(1 / al[np.arange(len(z)), y[rows]] - z.shape[1] / al.sum(1)) * num_bins
    return float(np.abs(g - np.round(g)).min()) if len(z) else 1.0


def cut_gap(scores, pos):
    """(top_m, score gap between the last negative inside the top-m cut and the first one outside)."""
    neg = np.sort(scores.reshape(-1)[~pos].astype(np.float64))
    top_m = min(int(pos.sum()), len(neg)) - 1
    return top_m, (float(neg[top_m] - neg[top_m - 1]) if 0 < top_m < len(neg) else np.inf)


def thumos_facts(heads, targets, priors, overlap=0.5, clip=256.0):
    out, tg = _t(heads, targets, priors)
    _, conf_t, _, pconf_t, iou_kb = O.match_anchors(out["loc"], out["priors"], tg, clip, overlap)
    conf_t, pconf_t = conf_t.reshape(-1).numpy(), pconf_t.reshape(-1).numpy()
    iou = iou_kb.transpose(0, 1).reshape(-1).numpy()        # batch-major, as conf_t
    return conf_t, pconf_t, iou


@pytest.mark.parametrize("name", list(LC.THUMOS_CASES))
def test_thumos_case_is_away_from_every_decision(name):
    heads, targets, priors = LC.thumos_case(name)
    B, K, C, _ = LC.THUMOS_CASES[name]
    A = B * K
    assert priors.shape[0] == K and heads["conf"].shape == (B, K, C) and all(1 <= len(t) <= 4 for t in targets)
    conf_t, pconf_t, iou = thumos_facts(heads, targets, priors)
    pos, ppos = conf_t > 0, pconf_t > 0
    assert pos.sum() > 0 and ppos.sum() > 0
    assert A > 1024 and pos[:1024].any() and pos[1024:].any() and ppos[:1024].any() and ppos[1024:].any()
    assert float(np.abs(iou[pos] - 0.5).min()) > 1e-5
    closed = C == 16
    for logits, tgt, keep in ((heads["conf"], conf_t, pos), (heads["prop_conf"], pconf_t, ppos)):
        rows = np.arange(A) if closed else np.nonzero(keep)[0]      # closed set: every anchor against its label (0 = background)
        y = tgt if closed else np.maximum(tgt - 1, 0)
        for nb in BIN_COUNTS:
            assert bin_margin(logits, y, rows, nb) > 1e-4, nb
    for scores, keep in ((heads["act"], pos), (heads["prop_act"], ppos)):
        top_m, gap = cut_gap(scores, keep)
        assert top_m > 0 and gap > 1e-6
    if not closed:          # the oracle itself runs the case: finite terms before and after ibm_start, and as the focal dispatch
        out, tg = _t(heads, targets, priors)
        for kind, epoch in (("edl", 0), ("edl", 12), ("focal", 0)):
            st = O.EvidenceState()
            st.epoch = epoch
            terms = O.multisegment_loss(out, tg, cls_loss_type=kind, state=st)
            assert all(np.isfinite(float(v)) for v in terms)


def test_thumos_rungs_match_the_kernel_limits():
    """The ladder's sizes against the constants of csrc/loss.hip: LT = 1024 threads, MAX_A = 2048, 96 KB of staged logits."""
    sizes = {n: b * k for n, (b, k, _, _) in LC.THUMOS_CASES.items()}
    assert all(n.endswith(str(a)) for n, a in sizes.items())
    assert min(sizes.values()) == 1025 and max(sizes.values()) == 2048
    stage = lambda n: sizes[n] * LC.THUMOS_CASES[n][2] * 4
    assert stage("open_1638") <= 96 * 1024 < stage("open_1764")         # C = 15: B = 13 staged, B = 14 not
    assert stage("closed_1512") <= 96 * 1024 < stage("closed_1638")     # C = 16: B = 12 staged, B = 13 not
    for r in LC.RUNGS:
        assert f"open_{r}" in sizes and f"closed_{r}" in sizes


def anet_facts(heads, targets, priors, overlap=0.6):
    """Per sample: (conf_t, prop_conf_t, iou, thr, margin of max(left, right) to the level bounds and of left / right to 0)."""
    res = []
    pri = torch.from_numpy(priors)
    for b in range(heads["loc"].shape[0]):
        gt = targets[b].astype(np.float64)
        c = priors[:, 0:1].astype(np.float64)
        left, right = (c - gt[None, :, 0]) * LC.ANET_CLIP, (gt[None, :, 1] - c) * LC.ANET_CLIP
        far = np.maximum(left, right)
        lb = np.array([LC.ANET_BOUNDS[int(l)][0] for l in priors[:, 1]], np.float64)[:, None]
        rb = np.array([LC.ANET_BOUNDS[int(l)][1] for l in priors[:, 1]], np.float64)[:, None]
        margin = min(np.abs(left).min(), np.abs(right).min(), np.abs(far - lb).min(), np.abs(far - rb).min())
        loc_t, pos = LC.anet_match(priors, targets[b])
        iou = O.tiou(torch.from_numpy(heads["loc"][b]), torch.from_numpy(loc_t)).numpy()
        thr = min(overlap, float(iou[pos].max()))
        ppos = pos & ~(iou < thr)
        res.append((pos, ppos, iou, thr, float(margin)))
    assert pri.shape[1] == 2
    return res


@pytest.mark.parametrize("K", list(LC.ANET_LEVELS))
def test_anet_case_is_away_from_every_decision(K):
    heads, targets, priors = LC.anet_inputs(K, 150)
    levels = LC.ANET_LEVELS[K]
    assert sum(levels) == K == priors.shape[0] and K <= 1024
    lvl = priors[:, 1].astype(int)
    for b, (pos, ppos, iou, thr, margin) in enumerate(anet_facts(heads, targets, priors)):
        assert margin > 1e-3                                    # no anchor on a segment's end or on a level bound
        for l in range(len(levels)):
            assert pos[lvl == l].any(), (b, l)                  # every level holds positives
        for k0 in range(0, K, 256):
            assert pos[k0:k0 + 256].any() and ppos[k0:k0 + 256].any(), (b, k0)      # and every 256-anchor sweep, in both stages
        assert thr == 0.6 and float(np.abs(iou[pos] - 0.6).min()) > 1e-5
        for scores, keep in ((heads["act"][b], pos), (heads["prop_act"][b], ppos)):
            top_m, gap = cut_gap(scores, keep)
            assert top_m > 0 and gap > 1e-6
    # the same inputs with the closed-set class count only differ in the logits
    h151, t151, _ = LC.anet_inputs(K, 151)
    assert all(np.array_equal(a, b) for a, b in zip(targets, t151)) and np.array_equal(h151["loc"], heads["loc"])
    # the oracle runs the case, with and without the influence-balanced weight, and matches what anet_match selected
    out, tg = _t(heads, targets, priors)
    for epoch in (0, 12):
        assert all(np.isfinite(float(v)) for v in O.multisegment_loss_anet(out, tg, cfg=arch.ANET, piou=0.6, epoch=epoch))


# ------------------------------------------------------------------------------------------------- the edge cases sit ON their edge
def _match(kind, heads, targets, priors):
    """The reference's matching of the one-sample edge cases: (loc_t, conf_t, prop_conf_t, iou), overlap threshold 0.5."""
    loc, pri, tg = torch.from_numpy(heads["loc"]), torch.from_numpy(priors), [torch.from_numpy(t) for t in targets]
    if kind == "thumos":
        from opental_amd.thumos14.multisegment_loss import MultiSegmentLoss
        crit = MultiSegmentLoss(15, 0.5, 1.0, cls_loss_type='focal', os_head=True, act_config=dict(margin=1.0, weight=0))
        ref = O.match_anchors(loc, pri, tg, 256.0, 0.5)
    else:
        from opental_amd.anet.multisegment_loss import MultiSegmentLoss
        crit = MultiSegmentLoss(150, 0.5, 1.0, cls_loss_type='focal', os_head=True)
        ref = None
    loc_t, conf_t, _, pconf_t, iou = crit.match(loc, pri, tg)
    if ref is not None:         # the package's batched matching IS the oracle's here, bit for bit
        assert torch.equal(ref[0], loc_t) and torch.equal(ref[1], conf_t) and torch.equal(ref[3], pconf_t)
        assert torch.equal(ref[4].transpose(0, 1), iou)
    return loc_t[0].numpy(), conf_t[0].numpy(), pconf_t[0].numpy(), iou[0].numpy()


@pytest.mark.parametrize("kind", ["thumos", "anet"])
def test_edge_cases_sit_exactly_on_their_edges(kind):
    # min / max ties
    heads, targets, priors, info = LC.edge_ties(kind)
    loc_t, conf_t, pconf_t, iou = _match(kind, heads, targets, priors)
    assert np.array_equal(loc_t[conf_t > 0], info["loc_t"][conf_t > 0])
    full, half = info["full"], info["half"]
    assert len(full) >= 3 and len(half) >= 3 and len(info["other"]) >= 2 and (conf_t[np.concatenate([full, half])] > 0).all()
    assert np.array_equal(heads["loc"][0, full], loc_t[full]) and (iou[full] == 1.0).all() and (heads["prop_loc"][0, full] == 0).all()
    assert np.array_equal(heads["loc"][0, half, 0], loc_t[half, 0]) and (heads["loc"][0, half, 1] > loc_t[half, 1]).all()
    # iou == thr
    heads, targets, priors, info = LC.edge_threshold(kind)
    loc_t, conf_t, pconf_t, iou = _match(kind, heads, targets, priors)
    x, y = info["x"], info["y"]
    assert iou[x] == np.float32(0.5) and 0.5 - 2e-7 < iou[y] < 0.5
    assert conf_t[x] > 0 and conf_t[y] > 0 and pconf_t[x] == conf_t[x] and pconf_t[y] == 0
    # clamp
    heads, targets, priors, info = LC.edge_clamp(kind)
    loc_t, conf_t, pconf_t, iou = _match(kind, heads, targets, priors)
    assert np.array_equal(conf_t[info["rows"]] > 0, info["is_pos"]) and np.array_equal(pconf_t, conf_t)
    v = LC.CLAMP_VALUES
    assert v[0] == 10 and v[1] > 10 and v[2] < 10 and v[4] == -10 and v[5] < -10 and v[6] > -10
    assert v[1] == np.nextafter(np.float32(10), np.float32(np.inf)) and v[5] == -v[1] and v[6] == -v[2]
    for name in ("conf", "prop_conf"):
        assert all(sorted(heads[name][0, r, :8]) == sorted(v) for r in info["rows"])
    # equal ground truths
    for variant in ("equal_area", "equal_area_swapped", "duplicate"):
        heads, targets, priors, info = LC.edge_ground_truths(kind, variant)
        loc_t, conf_t, _, _ = _match(kind, heads, targets, priors)
        g = targets[0]
        assert g[0, 1] - g[0, 0] == g[1, 1] - g[1, 0] and g[0, 2] != g[1, 2]
        assert len(info["both"]) >= 3 and (conf_t[info["both"]] == info["label"]).all()
    # the ranking of the negatives
    for variant in ("tie_straddle", "signed_zero", "all_equal", "npos1", "npos2"):
        heads, targets, priors, info = LC.edge_ranking(kind, variant)
        loc_t, conf_t, pconf_t, iou = _match(kind, heads, targets, priors)
        pos = conf_t > 0
        assert np.array_equal(pos, info["pos"]) and np.array_equal(pconf_t, conf_t)
        assert np.array_equal(heads["act"], heads["prop_act"])
        s = heads["act"][0, :, 0]
        neg = np.nonzero(~pos)[0]
        top_m = min(int(pos.sum()), len(neg)) - 1
        assert top_m == info["top_m"] == {"npos1": 0, "npos2": 1}.get(variant, top_m)
        assert s[info["top"]] == 3.0 and (np.delete(s[neg], np.nonzero(neg == info["top"])[0]) < 3.0).all()
        order = neg[np.argsort(s[neg], kind="stable")]
        if variant in ("tie_straddle", "signed_zero", "all_equal", "npos2"):
            assert top_m > 0 and s[order[top_m - 1]] == s[order[top_m]]                # the cut falls between two equal scores
        if variant == "signed_zero":
            group = neg[s[neg] == 0]
            sign = np.signbit(s[group])
            assert sign.any() and not sign.all() and group[sign].min() > group[~sign].max()     # -0.0 behind +0.0 by index
            assert not np.signbit(s[order[top_m - 1]]) and np.signbit(s[group]).sum() >= 6      # a -0.0-first order picks others
        # the oracle uses exactly the stable order's first top_m negatives (all of them when top_m <= 0)
        xs = torch.from_numpy(s.copy()).requires_grad_(True)
        loss, cnt = O.actionness_loss(xs.reshape(-1, 1), torch.from_numpy(pos.astype(np.float32)), 0.0)
        loss.backward()
        want = pos.copy()
        want[order[:top_m] if top_m > 0 else neg] = True
        assert int(cnt) == int(want.sum()) and np.array_equal(xs.grad.numpy() != 0, want)
