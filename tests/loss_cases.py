"""Deterministic inputs of the fused detection losses (csrc/loss.hip) past one sweep of their strided loops: the head outputs,
targets and priors of tests/test_loss_sweeps_gpu.py and tests/test_anet_loss_sweeps_gpu.py, as numpy arrays (no GPU code here).
tests/test_loss_cases_cpu.py runs every case under the CPU oracle alone and asserts that none of them sits near a decision of
the reference (bin edges, the overlap threshold, the top-m cut), so a GPU comparison cannot pass or fail by a coin flip; the
seeds below were picked until those conditions held.

THUMOS14 form: the recipe of tests/test_loss_gpu.py::_inputs (same draws in the same order), parameterised by the batch, the level
lengths, the class count and the seed.  ActivityNet form: the recipe of test_fused_anet_loss_equals_the_torch_formulation with
targets laid out so that every pyramid level and every 256-anchor sweep of a sample holds positives."""
import numpy as np

STD_LEVELS = (64, 32, 16, 8, 4, 2)                  # K = 126, the model's priors
# A = B * K rungs of the THUMOS14 kernel (LT = 1024 threads, MAX_A = 2048 anchors, 96 KB of staged logits)
LEVELS = {126: STD_LEVELS, 205: (104, 52, 26, 13, 6, 4), 128: (64, 32, 16, 8, 4, 4)}
# name -> (B, K, C, seed).  open: C = 15 logits (cls_mode 0 / 1 and the os_head ablations); closed: C = 16 (cls_mode 2 / 3, noACT, RPL)
THUMOS_CASES = {
    "open_1025": (5, 205, 15, 1), "open_1134": (9, 126, 15, 2), "open_1638": (13, 126, 15, 1), "open_1764": (14, 126, 15, 1),
    "open_2016": (16, 126, 15, 2), "open_2048": (16, 128, 15, 1),
    "closed_1025": (5, 205, 16, 2), "closed_1512": (12, 126, 16, 1), "closed_1638": (13, 126, 16, 5),
    "closed_1764": (14, 126, 16, 1), "closed_2016": (16, 126, 16, 1),
}
RUNGS = (1025, 1638, 1764, 2016)                    # every instance runs at these


def thumos_priors(levels):
    return np.concatenate([(np.arange(n, dtype=np.float64) + 0.5) / n for n in levels]).astype(np.float32).reshape(-1, 1)


def thumos_inputs(B, levels, C, seed):
    """(heads, targets, priors): heads = dict of float32 arrays (loc, conf, prop_loc, prop_conf, center, act, prop_act), targets =
    list of (n_i, 3) [start, end, label] with 1-4 rows per sample, priors (K, 1)."""
    rs = np.random.RandomState(seed)
    K = sum(levels)
    t = lambda *s, scale=1.0: (rs.randn(*s) * scale).astype(np.float32)
    loc = np.exp(rs.randn(B, K, 2) * 0.5 + 2.0).astype(np.float32)
    heads = dict(loc=loc, conf=t(B, K, C, scale=2.0), prop_loc=t(B, K, 2, scale=0.3), prop_conf=t(B, K, C, scale=2.0),
                 center=t(B, K, 1), act=t(B, K, 1), prop_act=t(B, K, 1))
    targets = []
    for i in range(B):
        rows = []
        for _ in range(1 + (i + seed) % 4):
            ln = rs.uniform(0.05, 0.5); st = rs.uniform(0, 1 - ln)
            rows.append([st, st + ln, float(rs.randint(1, 16))])
        targets.append(np.array(rows, np.float32).reshape(-1, 3))
    priors = thumos_priors(levels)
    if B * K == 1025:
        # the second trip of every loop is anchor 1024 alone: make it a positive of both stages (one target around the last
        # prior of the last sample, the coarse segment 10 % off on either side: tIoU ~ 0.87)
        c = float(priors[-1, 0])
        targets[-1] = np.array([[c - 0.26, c + 0.09, 7.0]], np.float32)
        loc[-1, -1] = (0.26 * 256 * 1.1, 0.09 * 256 * 0.9)
    return heads, targets, priors


def thumos_case(name):
    B, K, C, seed = THUMOS_CASES[name]
    return thumos_inputs(B, LEVELS[K], C, seed)


def as_distances(heads):
    """The RPL / GCPL instance reads conf / prop_conf as distances to the class centres: non-negative."""
    return dict(heads, conf=np.abs(heads["conf"]), prop_conf=np.abs(heads["prop_conf"]))


# ---------------------------------------------------------------------------------------------- ActivityNet1.3
ANET_CLIP = 768.0
ANET_BOUNDS = ((0, 30), (15, 60), (30, 120), (60, 240), (96, 768), (256, 768))     # anet/multisegment_loss.py bounds, frames
# K -> level lengths.  LQ = 256 anchors per sweep: 189 one sweep (the existing tests' size), 257 the smallest two-sweep case,
# 378 two, 1008 four, 1024 the limit (MAX_KA)
ANET_LEVELS = {189: (96, 48, 24, 12, 6, 3), 257: (128, 64, 32, 16, 8, 9), 378: (192, 96, 48, 24, 12, 6),
               1008: (512, 256, 128, 64, 32, 16), 1024: (512, 256, 128, 64, 32, 32)}
ANET_SEEDS = {189: 1, 257: 4, 378: 1, 1008: 1, 1024: 1}
# (start, length) in frames of the targets of sample 0 / 1: one long segment that the two coarsest levels accept everywhere,
# and shorter ones for the finer levels in both halves of the clip (levels 0 and 1 span more than one sweep at K >= 1008)
_ANET_SEGS = (
    ((20.95, 742.41), (100.95, 21.71), (501.35, 19.51), (200.85, 41.61), (611.05, 44.21), (301.25, 83.41), (400.75, 162.01),
     (381.55, 301.61)),
    ((15.25, 748.61), (61.55, 18.61), (660.85, 22.91), (121.05, 39.01), (560.95, 45.51), (221.45, 86.71), (331.15, 158.51),
     (251.35, 297.11)),
)


def anet_priors(levels):
    return np.concatenate([np.stack([(np.arange(t) + 0.5) / t, np.full(t, i)], 1) for i, t in enumerate(levels)]).astype(np.float32)


def anet_match(priors, gt):
    """The matching of anet/multisegment_loss.py:144-166 for one sample in float32 numpy (used only to draw `loc` near its target,
    so that the refined stage has more than one positive): (loc_t (K, 2), positive (K,))."""
    c = priors[:, 0:1]
    lb = np.array([ANET_BOUNDS[int(l)][0] for l in priors[:, 1]], np.float32)[:, None]
    rb = np.array([ANET_BOUNDS[int(l)][1] for l in priors[:, 1]], np.float32)[:, None]
    clip = np.float32(ANET_CLIP)
    left, right = (c - gt[None, :, 0]) * clip, (gt[None, :, 1] - c) * clip
    far = np.maximum(left, right)
    area = np.where((left < 0) | (right < 0) | (far <= lb) | (far > rb), clip * 2, left + right)
    best = area.argmin(1)
    k = np.arange(priors.shape[0])
    return np.stack([left[k, best], right[k, best]], 1), area[k, best] < clip * 2


def anet_inputs(K, C, seed=None, B=2):
    """(heads, targets, priors (K, 2)) for B <= 2 samples with `C` logits (150 open set, 151 closed set)."""
    levels = ANET_LEVELS[K]
    rs = np.random.RandomState(ANET_SEEDS[K] if seed is None else seed)
    priors = anet_priors(levels)
    targets = []
    for b in range(B):
        rows = [[s / ANET_CLIP, (s + ln) / ANET_CLIP, float(1 + (17 * g + 5 * b) % 150)] for g, (s, ln) in enumerate(_ANET_SEGS[b])]
        targets.append(np.array(rows, np.float32))
    mk = lambda *shape, scale=1.0: (rs.randn(*shape) * scale).astype(np.float32)
    loc = (np.abs(rs.randn(B, K, 2)) * 40 + 5).astype(np.float32)
    near = rs.randn(B, K, 2)
    for b in range(B):          # a positive's coarse segment: its target, off by a log-normal factor (tIoU on both sides of 0.6)
        loc_t, pos = anet_match(priors, targets[b])
        loc[b][pos] = (np.maximum(loc_t[pos], 0.5) * np.exp(0.7 * near[b][pos])).astype(np.float32)
    heads = dict(loc=loc, conf=mk(B, K, C, scale=2.0), prop_loc=mk(B, K, 2, scale=0.8), prop_conf=mk(B, K, C, scale=2.0),
                 center=mk(B, K, 1), act=mk(B, K, 1), prop_act=mk(B, K, 1))
    return heads, targets, priors


# ---------------------------------------------------------------------------------------------- decision edges
# Inputs of tests/test_loss_edges_gpu.py: built from dyadic rationals (priors (k + 1/2) / 2^n, target ends in 1/512, head outputs
# in 1/4 or 1/8), so every quantity a DECISION depends on -- left / right extents, areas, tIoU of the constructed anchors -- is
# exact in float32 and the same in the kernel, the torch formulation and the oracle.  kind: "thumos" (K = 126, 256 frames, C = 15)
# or "anet" (dyadic level lengths, K = 252, 768 frames, C = 150).
EDGE = {"thumos": dict(levels=STD_LEVELS, clip=256.0, C=15), "anet": dict(levels=(128, 64, 32, 16, 8, 4), clip=768.0, C=150)}
CLAMP_VALUES = np.array([10.0, np.nextafter(np.float32(10), np.float32(11)), np.nextafter(np.float32(10), np.float32(9)), 30.0,
                         -10.0, np.nextafter(np.float32(-10), np.float32(-11)), np.nextafter(np.float32(-10), np.float32(-9)), -30.0],
                        np.float32)      # at the clamp, one float outside, one inside, far outside; both signs


def _dyadic(rs, shape, lo, hi, q=4):
    return (rs.randint(lo * q, hi * q + 1, shape) / q).astype(np.float32)


def edge_priors(kind):
    lv = EDGE[kind]["levels"]
    return thumos_priors(lv) if kind == "thumos" else anet_priors(lv)


def edge_match(kind, priors, gt):
    """(loc_t (K, 2), label (K,)) of one sample, float32, first minimum among equal areas (targets all valid)."""
    clip = np.float32(EDGE[kind]["clip"])
    if kind == "anet":
        loc_t, pos = anet_match(priors, gt)
    else:
        c = priors[:, 0:1]
        left, right = (c - gt[None, :, 0]) * clip, (gt[None, :, 1] - c) * clip
        area = np.where((left < 0) | (right < 0), clip * 2, left + right)
        best = area.argmin(1)
        k = np.arange(priors.shape[0])
        loc_t, pos = np.stack([left[k, best], right[k, best]], 1), area[k, best] < clip * 2
    c = priors[:, 0:1]
    clipv = np.float32(EDGE[kind]["clip"])
    lab = np.zeros(priors.shape[0], np.int64)
    for k in np.nonzero(pos)[0]:        # the row whose extents are loc_t[k]: the first one
        for g in range(gt.shape[0]):
            if (c[k, 0] - gt[g, 0]) * clipv == loc_t[k, 0] and (gt[g, 1] - c[k, 0]) * clipv == loc_t[k, 1]:
                lab[k] = int(gt[g, 2])
                break
    return loc_t.astype(np.float32), lab


def edge_heads(kind, seed, B=1):
    """Dyadic head outputs; the actionness scores are continuous draws (no accidental tie at the top-m cut)."""
    rs = np.random.RandomState(seed)
    K, C = sum(EDGE[kind]["levels"]), EDGE[kind]["C"]
    return dict(loc=_dyadic(rs, (B, K, 2), 1, 40), conf=_dyadic(rs, (B, K, C), -4, 4), prop_loc=_dyadic(rs, (B, K, 2), -1, 1, 8),
                prop_conf=_dyadic(rs, (B, K, C), -4, 4), center=_dyadic(rs, (B, K, 1), -2, 2),
                act=rs.randn(B, K, 1).astype(np.float32), prop_act=rs.randn(B, K, 1).astype(np.float32))


def _seg(a, b, label):
    return [a / 512.0, b / 512.0, float(label)]


def edge_ties(kind):
    """min / max ties of the tIoU terms.  Of the positives of one target, every third has loc == loc_t and prop_loc == 0 (tIoU = 1:
    every min and max of the GIoU term AND of the quality head's refined segment ties, and the refined L1 error is exactly 0),
    every third has only its left side equal, the rest is off on both sides.  info: indices of the three groups."""
    heads = edge_heads(kind, 41)
    priors = edge_priors(kind)
    targets = [np.array([_seg(128, 384, 3)] if kind == "thumos" else [_seg(128, 256, 3)], np.float32)]
    loc_t, lab = edge_match(kind, priors, targets[0])
    p = np.nonzero(lab > 0)[0]
    full, half = p[0::3], p[1::3]
    heads["loc"][0, full] = loc_t[full]
    heads["prop_loc"][0, full] = 0.0
    heads["loc"][0, half, 0] = loc_t[half, 0]
    heads["loc"][0, half, 1] = loc_t[half, 1] * 2 + 1
    return heads, targets, priors, dict(full=full, half=half, other=p[2::3], loc_t=loc_t)


def edge_threshold(kind):
    """iou < thr at equality.  Two targets, each around ONE finest-level prior with extents (d, d) frames: anchor X predicts (2d, 2d)
    -- tIoU = 2d / 4d = 0.5 exactly, not below the threshold 0.5: it stays a refined-stage positive -- and anchor Y predicts
    (2d, 2d + a few ulps): tIoU is the nearest value below 0.5 this arithmetic reaches, and it does not.  info: x, y."""
    heads = edge_heads(kind, 42)
    priors = edge_priors(kind)
    n0 = EDGE[kind]["levels"][0]
    kx, ky = 10, 40
    unit = 512 // (2 * n0)                  # half a finest-level spacing, in 1/512: the prior is (2 k + 1) * unit
    half = unit if kind == "thumos" else unit      # target = prior +- half a spacing
    rows = [_seg((2 * k + 1) * unit - half, (2 * k + 1) * unit + half, lab) for k, lab in ((kx, 4), (ky, 9))]
    targets = [np.array(rows, np.float32)]
    loc_t, lab = edge_match(kind, priors, targets[0])
    d = float(loc_t[kx, 0])
    assert tuple(loc_t[kx]) == (d, d) == tuple(loc_t[ky]) and lab[kx] == 4 and lab[ky] == 9
    heads["loc"][0, kx] = (2 * d, 2 * d)
    up = np.float32(2 * d)
    for _ in range(4):
        up = np.nextafter(up, np.float32(1e9))
    heads["loc"][0, ky] = (2 * d, up)
    return heads, targets, priors, dict(x=kx, y=ky, d=d, loc_t=loc_t, lab=lab)


def edge_clamp(kind):
    """Logits at the clamp of exp(clamp(z, -10, 10)): CLAMP_VALUES rotated through the first columns (so that the label's column
    meets each of them) of three positive and three negative rows of conf and prop_conf; the positives predict their target
    exactly (tIoU = 1), so they are positives of both stages.  info: rows (6,), is_pos (6,)."""
    heads = edge_heads(kind, 43)
    priors = edge_priors(kind)
    targets = [np.array([_seg(128, 384, 3)] if kind == "thumos" else [_seg(128, 256, 3)], np.float32)]
    loc_t, lab = edge_match(kind, priors, targets[0])
    p, n = np.nonzero(lab > 0)[0], np.nonzero(lab == 0)[0]
    heads["loc"][0, p] = np.maximum(loc_t[p], 0.25)
    heads["loc"][0, p[loc_t[p].min(1) > 0]] = loc_t[p[loc_t[p].min(1) > 0]]
    rows = np.concatenate([p[[1, 2, 3]], n[[0, 5, 9]]])
    for j, r in enumerate(rows):
        for name in ("conf", "prop_conf"):
            heads[name][0, r, :8] = np.roll(CLAMP_VALUES, j + (name == "prop_conf"))
    return heads, targets, priors, dict(rows=rows, is_pos=np.array([1, 1, 1, 0, 0, 0], bool), loc_t=loc_t, lab=lab)


def edge_ground_truths(kind, variant):
    """"equal_area": two targets of the same length overlap, the anchors inside both see two equal areas: the FIRST row wins
    (label 3); "equal_area_swapped": the rows the other way round (label 5 wins); "duplicate": the same segment twice with
    labels 3 and 9: label 3.  info: both = the anchors that either target alone would win, label = the label they must get."""
    heads = edge_heads(kind, 44)
    priors = edge_priors(kind)
    a, b = (_seg(128, 256, 3), _seg(192, 320, 5))
    rows = {"equal_area": [a, b], "equal_area_swapped": [b, a], "duplicate": [a, _seg(128, 256, 9)]}[variant]
    targets = [np.array(rows, np.float32)]
    loc_t, lab = edge_match(kind, priors, targets[0])
    alone = [edge_match(kind, priors, targets[0][g:g + 1])[1] > 0 for g in range(2)]       # (per-level bounds: ActivityNet)
    both = np.nonzero(alone[0] & alone[1])[0]
    return heads, targets, priors, dict(both=both, label=int(rows[0][2]), lab=lab, loc_t=loc_t)


def edge_ranking(kind, variant):
    """The negative ranking of the positive-unlabelled actionness loss: ascending score, then lower anchor index; the first
    top_m = min(P, N) - 1 negatives are used.  act and prop_act carry the same scores and every positive predicts its target
    exactly, so both passes rank the same set.  One negative (info['top']) holds the unique largest score (the rank hinge of the
    ActivityNet recipe differentiates the maximum).
      "tie_straddle"  scores -1 / 0.5 / 2 by index pattern: the cut falls inside the group of 0.5s
      "signed_zero"   the same with the group at zero: +0.0 at its lower indices, -0.0 at its higher ones -- equal scores
      "all_equal"     every other negative at 0.25
      "npos1"         one positive: top_m = 0, every negative is used;  "npos2": two positives: exactly one negative"""
    heads = edge_heads(kind, 45)
    priors = edge_priors(kind)
    n0 = EDGE[kind]["levels"][0]
    unit = 512 // (2 * n0)
    one = lambda k, lab: _seg((2 * k + 1) * unit - unit // 2, (2 * k + 1) * unit + unit // 2, lab)     # holds one prior only
    if variant == "npos1":
        rows = [one(7, 2)]
    elif variant == "npos2":
        rows = [one(7, 2), one(33, 6)]
    else:
        rows = [_seg(128, 256, 3)]
    targets = [np.array(rows, np.float32)]
    loc_t, lab = edge_match(kind, priors, targets[0])
    pos = lab > 0
    heads["loc"][0, pos] = np.maximum(loc_t[pos], 0.25)
    neg = np.nonzero(~pos)[0]
    top_m = min(int(pos.sum()), len(neg)) - 1
    s = heads["act"][0, :, 0]
    s[pos] = _dyadic(np.random.RandomState(5), (int(pos.sum()),), -2, 2)
    if variant in ("tie_straddle", "signed_zero"):
        tie = 0.5 if variant == "tie_straddle" else 0.0
        low = max(top_m - 6, 1)                                 # `low` scores below the group: the cut takes 6 of the tied ones
        vals = np.full(len(neg), 2.0, np.float32)
        order = np.random.RandomState(6).permutation(len(neg))
        vals[order[:low]] = -1.0
        group = np.sort(order[low:low + 14])
        vals[group] = tie
        if variant == "signed_zero":
            vals[group[7:]] = -0.0
        s[neg] = vals
    elif variant == "all_equal":
        s[neg] = 0.25
    else:                   # npos1 / npos2: dyadic scores with the two lowest tied
        vals = _dyadic(np.random.RandomState(7), (len(neg),), -1, 2)
        vals[[11, 60]] = -1.5
        s[neg] = vals
    s[neg[-3]] = 3.0
    heads["prop_act"][0, :, 0] = s
    return heads, targets, priors, dict(pos=pos, top_m=top_m, top=int(neg[-3]), lab=lab, loc_t=loc_t)
