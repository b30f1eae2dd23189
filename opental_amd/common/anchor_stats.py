"""The anchor diagnostics of a trained THUMOS14 detector, before decoding and Soft-NMS, as one rule over (B, K, .) head outputs.

Three scripts of the reference look at the anchors this way, all through one function, get_matched_targets, copied into each:
experiments/analyze_actionness.py:226-339 (a score per anchor and stage, split by the matched label into known / unknown /
background), AFSD/thumos14/draw_distribution.py:221-258,:323-389 (the same split, known against the rest) and
experiments/analyze_gradnorm.py:124-189,:248-271 (the EDL gradient 1/alpha_y - C/S of the anchors that count in the loss and
its density over 100 bins).  They save every head output to disk and loop over windows on the host; here it is one launch
per batch of windows and only histograms leave the device.

  * `anchor_stats_reference` -- the rule in plain numpy: the oracle of otal_anchor_stats (csrc/anchorstats.hip) and the form
    that serves host tensors;
  * `anchor_stats` -- device tensors through the kernel (ops.anchor_stats), host tensors through `anchor_stats_reference`.

Inputs in the layouts of the detection loss: loc (B, K, 2) frames; conf, prop_conf (B, K, C) logits; center (B, K); act,
prop_act (B, K) or both None; priors (K); gt (B, G, 3) = [start, end, label] in units of the clip, padded, with gvalid (B, G).

Matching (get_matched_targets): the coarse label is phase 1 of the loss kernel -- the first minimum of left + right over the
valid ground truths that contain the anchor, 0 when none does; the refined label is the coarse one, 0 where the IoU of loc
with the matched target is below `overlap_thresh` (compute_iou, eps-clamped union).  float32, the loss kernel's operations
in its order, so labels are exact.  A sample with no valid ground truth is all background (the unannotated windows of
draw_distribution.py:357-369).

Groups per stage (analyze_actionness.py:323-325), GROUPS: known = labels 1..n_known, unknown = labels above, background = 0.

Score per stage (get_result, analyze_actionness.py:266-295), TARGETS, with alpha = exp(clamp(z, +-10)) + 1, S = sum alpha:
uncertainty C / S; actionness sigmoid(the stage's actionness logit); confidence max_k (alpha_k / S) sigmoid(center), times the
actionness with os_head; uncertainty_actionness; half_au = 0.5 (actionness + 1) uncertainty.  draw_distribution.py:329
multiplies by the RAW actionness map; this rule follows analyze_actionness.py:271, where it is a sigmoid.  The three targets
that use the actionness need os_head; softmax heads are refused (the reference computes gradients for 'edl' only).

EDL gradient per stage (grad_edl, analyze_gradnorm.py:173-189): g = 1/alpha_y - C/S at the label's column.  With os_head the
rows that count are the anchors labelled 1..C at column y - 1 (:218-221); without it every anchor at column y, 0 =
background (the loss's cls_mode 2).  A label outside the head's columns gives no row; rows that do not count hold 0.

Histograms are integer counts ADDED to what the arrays hold: hist_score int64 (2 stages, 3 groups, score_bins) with bin
min((int)floorf(v * (float)score_bins), score_bins - 1) in float32, a NaN score counted nowhere; hist_grad int64 (2,
grad_bins) over |g| with the bins of plot_grad_density (edges i / grad_bins, the last + 1e-6; the loss's reweight 2)."""
import numpy as np
import torch

TARGETS = ('uncertainty', 'actionness', 'confidence', 'uncertainty_actionness', 'half_au')     # the kernel's `target` = the index
ACT_TARGETS = ('actionness', 'uncertainty_actionness', 'half_au')
STAGES = ('coarse', 'refined')
GROUPS = ('known', 'unknown', 'background')
F32_EPS = np.float32(np.finfo(np.float32).eps)


def check_mode(target, os_head, use_edl=True, have_act=None):
    """The refusals of the rule, before anything is computed."""
    if target not in TARGETS:
        raise NotImplementedError(f"target {target!r}: one of {TARGETS}")
    if not use_edl:
        raise NotImplementedError("softmax heads: the anchor statistics are those of an evidential head (use_edl)")
    if target in ACT_TARGETS and not os_head:
        raise NotImplementedError(f"target {target!r} needs the actionness maps of os_head")
    if have_act is not None and os_head and not have_act:
        raise RuntimeError("os_head without act / prop_act")


def score_edges(bins):
    return np.arange(bins + 1, dtype=np.float64) / bins


def grad_edges(bins):
    """The edges of plot_grad_density as the float32 numbers a float32 gradient is compared with."""
    e = [float(x) / bins for x in range(bins + 1)]
    e[-1] += 1e-6
    return np.array(e, dtype=np.float64).astype(np.float32)


def group_of(label, n_known):
    """GROUPS index of every label."""
    label = np.asarray(label)
    return np.where(label == 0, 2, np.where(label <= n_known, 0, 1)).astype(np.int32)


def match_reference(loc, priors, gt, gvalid, clip_length, overlap_thresh):
    """get_matched_targets in float32 -> label int32 (B, K, 2), and for the tests' margins iou (B, K) and area_gap (B, K), the
    difference of the two smallest candidate areas of an anchor (inf with one ground truth)."""
    loc = np.asarray(loc, np.float32)
    priors = np.asarray(priors, np.float32).reshape(-1)
    gt = np.asarray(gt, np.float32)
    gvalid = np.asarray(gvalid).astype(bool)
    B, K = loc.shape[:2]
    clip, big = np.float32(clip_length), np.float32(clip_length) * np.float32(2)
    label = np.zeros((B, K, 2), np.int32)
    iou = np.zeros((B, K), np.float32)
    gap = np.full((B, K), np.inf, np.float32)
    c = priors[:, None]
    rows = np.arange(K)
    with np.errstate(invalid='ignore', divide='ignore'):
        for b in range(B):
            left = (c - gt[b, None, :, 0]) * clip
            right = (gt[b, None, :, 1] - c) * clip
            area = left + right
            area = np.where((left < 0) | (right < 0) | ~gvalid[b][None, :], big, area).astype(np.float32)
            best = area.argmin(1)                                   # the first minimum, like torch.min
            best_area = area[rows, best]
            if area.shape[1] > 1:
                two = np.sort(area, 1)[:, :2]
                gap[b] = two[:, 1] - two[:, 0]
            lt0 = (priors - gt[b, best, 0]) * clip
            lt1 = (gt[b, best, 1] - priors) * clip
            coarse = np.where(best_area >= big, 0, gt[b, best, 2].astype(np.int32))
            p0, p1 = loc[b, :, 0], loc[b, :, 1]
            inter = np.minimum(p0, lt0) + np.minimum(p1, lt1)
            uni = (lt0 + lt1) + (p0 + p1) - inter
            iou[b] = inter / np.maximum(uni, F32_EPS)
            label[b, :, 0] = coarse
            label[b, :, 1] = np.where(iou[b] < np.float32(overlap_thresh), 0, coarse)
    return label, iou, gap


def _sigmoid(x):
    with np.errstate(over='ignore'):
        return (np.float32(1) / (np.float32(1) + np.exp(-np.asarray(x, np.float32)))).astype(np.float32)


def grad_bin(g, bins):
    """The bin of every |g| under plot_grad_density's edges, -1 where none holds it."""
    edges = grad_edges(bins)
    b = np.searchsorted(edges, g, side='right') - 1                 # edges[b] <= g < edges[b + 1]
    return np.where((b >= 0) & (b < bins) & ~np.isnan(g), b, -1)


def score_bin(v, bins):
    """The bin of every score, -1 for a NaN."""
    with np.errstate(invalid='ignore'):
        x = np.floor(np.asarray(v, np.float32) * np.float32(bins))
        b = np.clip(np.nan_to_num(x, nan=0.0, posinf=bins - 1, neginf=0.0), 0, bins - 1).astype(np.int64)
    return np.where(np.isnan(v), -1, b)


def alpha_of(z, evidence='exp'):
    """alpha = evidence(z) + 1 in float32 (DirichletLayer.evidence_func; csrc/evidence.h)."""
    z = np.asarray(z, np.float32)
    one = np.float32(1)
    if evidence == 'exp':
        return (np.exp(np.clip(z, np.float32(-10), np.float32(10))) + one).astype(np.float32)
    if evidence == 'relu':
        return (np.maximum(z, np.float32(0)) + one).astype(np.float32)
    if evidence == 'softplus':
        with np.errstate(over='ignore'):
            return (np.where(z > np.float32(20), z, np.log1p(np.exp(z))) + one).astype(np.float32)
    raise NotImplementedError(f"evidence {evidence!r}")


def anchor_stats_reference(loc, conf, prop_conf, center, act, prop_act, priors, gt, gvalid, clip_length, overlap_thresh,
                           os_head, n_known, target, score_bins=100, grad_bins=100, use_edl=True, hist_score=None,
                           hist_grad=None, evidence='exp'):
    """The rule on host arrays -> dict(label int32, value fp32, grad fp32, counts bool (B, K, 2): the rows of the gradient;
    group int32 (B, K, 2): GROUPS index; hist_score, hist_grad int64 (added to the arrays passed in, or fresh); iou, area_gap:
    match_reference's margins).  Sums over the classes run in float32 in the order of the columns, as the kernel's.
    evidence: the network's evidence function ('exp', 'relu', 'softplus'; grad_edl, analyze_gradnorm.py:164-184)."""
    check_mode(target, os_head, use_edl, have_act=act is not None and prop_act is not None)
    if int(n_known) < 1 or score_bins < 1 or grad_bins < 1:
        raise ValueError("n_known, score_bins and grad_bins are at least 1")
    conf, prop_conf = np.asarray(conf, np.float32), np.asarray(prop_conf, np.float32)
    B, K, C = conf.shape
    label, iou, gap = match_reference(loc, priors, gt, gvalid, clip_length, overlap_thresh)
    ct = _sigmoid(np.asarray(center, np.float32).reshape(B, K))
    value = np.zeros((B, K, 2), np.float32)
    grad = np.zeros((B, K, 2), np.float32)
    counts = np.zeros((B, K, 2), bool)
    hist_score = np.zeros((2, 3, score_bins), np.int64) if hist_score is None else hist_score
    hist_grad = np.zeros((2, grad_bins), np.int64) if hist_grad is None else hist_grad
    group = group_of(label, n_known)
    for s, (z, a) in enumerate(((conf, act), (prop_conf, prop_act))):
        alpha = alpha_of(z, evidence)
        S = np.zeros((B, K), np.float32)
        for k in range(C):
            S = S + alpha[:, :, k]
        u = np.float32(C) / S
        an = None if a is None else _sigmoid(np.asarray(a, np.float32).reshape(B, K))
        if target == 'uncertainty':
            v = u
        elif target == 'actionness':
            v = an
        elif target == 'confidence':
            v = alpha / S[:, :, None] * ct[:, :, None]
            if os_head:
                v = v * an[:, :, None]
            v = v.max(-1)
        elif target == 'uncertainty_actionness':
            v = u * an
        else:
            v = np.float32(0.5) * (an + np.float32(1)) * u
        value[:, :, s] = v
        col = label[:, :, s] - 1 if os_head else label[:, :, s]
        ok = (col >= 0) & (col < C)
        ay = np.take_along_axis(alpha, np.clip(col, 0, C - 1)[:, :, None], 2)[:, :, 0]
        grad[:, :, s] = np.where(ok, np.float32(1) / ay - u, np.float32(0))
        counts[:, :, s] = ok
        sb = score_bin(value[:, :, s], score_bins)
        for g in range(3):
            m = (group[:, :, s] == g) & (sb >= 0)
            hist_score[s, g] += np.bincount(sb[m], minlength=score_bins)
        gb = grad_bin(np.abs(grad[:, :, s]), grad_bins)
        hist_grad[s] += np.bincount(gb[ok & (gb >= 0)], minlength=grad_bins)
    return dict(label=label, value=value, grad=grad, counts=counts, group=group, hist_score=hist_score, hist_grad=hist_grad,
                iou=iou, area_gap=gap)


def anchor_stats(loc, conf, prop_conf, center, act, prop_act, priors, gt, gvalid, clip_length, overlap_thresh, os_head, n_known,
                 target, score_bins=100, grad_bins=100, use_edl=True, out=None, rows=True, evidence='exp'):
    """The statistics of a batch of windows: device tensors go through otal_anchor_stats / otal_anchor_stats_ev (`out`, `rows`:
    ops.anchor_stats), host tensors through `anchor_stats_reference` (returned as host tensors; out['hist_score'] /
    out['hist_grad'] are added to).  evidence: the network's evidence function."""
    check_mode(target, os_head, use_edl, have_act=act is not None and prop_act is not None)
    if conf.is_cuda:
        from . import ops
        return ops.anchor_stats(loc, conf, prop_conf, center, act, prop_act, priors, gt, gvalid, clip_length, overlap_thresh,
                                os_head, n_known, target, score_bins, grad_bins, out=out, rows=rows, evidence=evidence)
    npy = lambda t: None if t is None else t.detach().numpy()
    hs = None if out is None else out['hist_score'].numpy()
    hg = None if out is None else out['hist_grad'].numpy()
    ref = anchor_stats_reference(npy(loc), npy(conf), npy(prop_conf), npy(center), npy(act), npy(prop_act), npy(priors), npy(gt),
                                 npy(gvalid), clip_length, overlap_thresh, os_head, n_known, target, score_bins, grad_bins,
                                 hist_score=hs, hist_grad=hg, evidence=evidence)
    keys = ('hist_score', 'hist_grad') + (('label', 'value', 'grad') if rows else ())
    res = {k: torch.as_tensor(ref[k]) for k in keys}
    for k in ('label', 'value', 'grad'):
        res.setdefault(k, None)
    return res
