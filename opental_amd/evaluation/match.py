"""The greedy prediction -> ground-truth matching of the detection evaluation, stated once.

Both loops of eval_detection.py (split_results_by_gt for AUROC / AUPR / FAR@95 / OSDR, compute_average_precision_detection
for mAP; reference AFSD/evaluation/eval_detection.py:405-456 and :323-402) reduce to one rule.  A *group* is an ordered list
of predictions, the group's ground-truth segments and one tIoU threshold `thr`.  Predictions are visited in order; a ground
truth can be taken once.  For prediction i, with tiou_j its fp64 tIoU (utils_eval.segment_iou) against ground truth j:

  * if an untaken j with `not (tiou_j < thr)` exists, i MATCHES the one with the largest tIoU -- the lowest row among equal
    tIoU -- and that ground truth becomes taken; the result is the ground truth's row;
  * otherwise, if any j has `tiou_j < thr`, the result is -1 ('bg' in the split pass, a false positive in the AP pass);
  * otherwise the result is -2: every ground truth clears the threshold and all are taken (split_results_by_gt appends such
    a prediction to no list; the AP pass counts a false positive);
  * a group without ground truth gives -1 for every prediction.

Thresholds are independent problems with their own taken-sets.  Ties: the CPU loops take whichever of two equal tIoU
`argsort()[::-1]` lists first, which depends on the numpy build; the rule here is deterministic (lowest row).

match_reference is the executable statement of the rule in numpy (the oracle of the GPU tests and the fallback),
match_device the same through otal_eval_match (csrc/eval.hip).  plan_split / plan_ap turn the evaluator's column arrays
into group-sorted arrays and map the results back; they are vectorised, no per-row Python.

Labelled matching (the Wilderness-Impact pass, compute_wilderness_impact :604-728) is a second rule beside it.  A group is a
video: its predictions in file order, its ground truths of ALL classes, the unknown label 0 included; predictions and ground
truths carry labels.  For prediction i with label lp:

  * MATCH as above: among the ground truths that are not locked and satisfy `not (tiou_j < thr)` the one with the largest
    tIoU, the lowest row among equal tIoU; the result is its row;
  * LOCK: that ground truth becomes locked only where lp == label_j, a true positive (:676-681 writes lock_gt in the TP
    branch alone).  A false positive leaves it open for later predictions -- the one difference from the rule above;
  * without a candidate the result is -1 where some tiou_j < thr (the background break, :662-667) and -2 where every ground
    truth clears the threshold and is locked (the reference sets no flag for such a prediction); a group without ground
    truth gives -1 (the reference cannot have one, the planner can);
  * once per prediction, whatever the threshold: max_tiou = the largest tIoU over the group's ground truths (:656), 0 for a
    group without ground truth.

Ties are decided as above, by the lowest row, where the reference's `argsort()[::-1]` leaves them to the numpy build; they
arise only between ground truths with equal tIoU at or above the threshold, that is duplicated ground-truth segments.
match_labeled_reference is this rule in numpy, match_labeled_device the same through otal_eval_match_labeled; plan_split's
Plan serves both rules (group = video, file order) and its order / gt_order carry the labels.  wi_outcome_codes / wi_outcomes
turn result codes and the two labels into the pass's seven outcomes, on the host."""
import warnings

import numpy as np

from .utils_eval import segment_iou

MAX_THRESHOLDS = 32


def match_reference(pred_seg, pred_start, gt_seg, gt_start, thresholds):
    """pred_seg (N, 2), gt_seg (M, 2) sorted by group; *_start (ngroups + 1) offsets -> int32 (nthr, N): the matched row of
    gt_seg, -1 or -2 (module docstring)."""
    pred_seg = np.asarray(pred_seg, dtype=np.float64).reshape(-1, 2)
    gt_seg = np.asarray(gt_seg, dtype=np.float64).reshape(-1, 2)
    thr = np.asarray(thresholds, dtype=np.float64).reshape(-1)
    out = np.full((len(thr), len(pred_seg)), -1, dtype=np.int32)
    for g in range(len(pred_start) - 1):
        g0, g1 = int(gt_start[g]), int(gt_start[g + 1])
        if g1 == g0:
            continue
        segs = gt_seg[g0:g1]
        taken = np.zeros((len(thr), g1 - g0), dtype=bool)
        for i in range(int(pred_start[g]), int(pred_start[g + 1])):
            with np.errstate(invalid='ignore', divide='ignore'):
                tiou = segment_iou(pred_seg[i], segs)
                below = tiou[None, :] < thr[:, None]
            cand = ~below & ~taken
            # np.argmax returns the first maximum: the lowest row among equal tIoU
            best = np.where(cand, tiou[None, :], -np.inf).argmax(axis=1)
            hit = cand.any(axis=1)
            out[:, i] = np.where(hit, g0 + best, np.where(below.any(axis=1), -1, -2))
            taken[hit, best[hit]] = True
    return out


def match_labeled_reference(pred_seg, pred_label, pred_start, gt_seg, gt_label, gt_start, thresholds):
    """The labelled rule (module docstring).  Arrays as match_reference's, pred_label (N) / gt_label (M) integer labels in
    the rows' order -> (int32 codes (nthr, N): the matched row of gt_seg, -1 or -2; fp64 max_tiou (N))."""
    pred_seg = np.asarray(pred_seg, dtype=np.float64).reshape(-1, 2)
    gt_seg = np.asarray(gt_seg, dtype=np.float64).reshape(-1, 2)
    pred_label, gt_label = np.asarray(pred_label).reshape(-1), np.asarray(gt_label).reshape(-1)
    thr = np.asarray(thresholds, dtype=np.float64).reshape(-1)
    out = np.full((len(thr), len(pred_seg)), -1, dtype=np.int32)
    max_tiou = np.zeros(len(pred_seg), dtype=np.float64)
    for g in range(len(pred_start) - 1):
        g0, g1 = int(gt_start[g]), int(gt_start[g + 1])
        if g1 == g0:
            continue
        segs, labels = gt_seg[g0:g1], gt_label[g0:g1]
        locked = np.zeros((len(thr), g1 - g0), dtype=bool)
        for i in range(int(pred_start[g]), int(pred_start[g + 1])):
            with np.errstate(invalid='ignore', divide='ignore'):
                tiou = segment_iou(pred_seg[i], segs)
                below = tiou[None, :] < thr[:, None]
            max_tiou[i] = tiou.max()
            cand = ~below & ~locked
            # np.argmax returns the first maximum: the lowest row among equal tIoU
            best = np.where(cand, tiou[None, :], -np.inf).argmax(axis=1)
            hit = cand.any(axis=1)
            out[:, i] = np.where(hit, g0 + best, np.where(below.any(axis=1), -1, -2))
            tp = hit & (labels[best] == pred_label[i])
            locked[tp, best[tp]] = True
    return out, max_tiou


WI_OUTCOMES = ('tp_u2u', 'tp_k2k', 'fp_u2k', 'fp_k2k', 'fp_k2u', 'fp_bg2u', 'fp_bg2k')
WI_PER_CLASS = ('tp_k2k', 'fp_u2k', 'fp_k2k', 'fp_bg2k')       # (T, K, N) arrays, the class = the PREDICTION's label - 1


def wi_outcome_codes(codes, pred_label, gt_label):
    """Result codes (nthr, N) of the labelled rule, pred_label (N) and gt_label (M; codes >= 0 index it) -> int8 (nthr, N):
    the index into WI_OUTCOMES of each prediction's outcome (compute_wilderness_impact :662-689), -1 for none (code -2).
    Label 0 is '__unknown__'."""
    codes = np.asarray(codes)
    lp = np.asarray(pred_label, dtype=np.int64).reshape(1, -1)
    gt_label = np.asarray(gt_label, dtype=np.int64).reshape(-1)
    lg = gt_label[np.maximum(codes, 0)] if len(gt_label) else np.zeros(codes.shape, dtype=np.int64)
    matched = codes >= 0
    fp = np.where(lg == 0, 2, np.where(lp == 0, 4, 3))                          # fp_u2k, fp_k2u, fp_k2k
    outcome = np.where(matched, np.where(lp == lg, np.where(lg == 0, 0, 1), fp),
                       np.where(codes == -1, np.where(lp == 0, 5, 6), -1))
    return outcome.astype(np.int8)


def wi_outcomes(codes, pred_label, gt_label, n_known):
    """The seven outcome arrays of compute_wilderness_impact in its shapes, as 0 / 1 in fp64: dict of WI_OUTCOMES ->
    (nthr, N), or (nthr, n_known, N) for WI_PER_CLASS.  A prediction has at most one flag, none for code -2; these are the
    flags as the pass sets them, before it folds the background ones into fp_k2u / fp_k2k (:712-713)."""
    outcome = wi_outcome_codes(codes, pred_label, gt_label)
    lp = np.asarray(pred_label, dtype=np.int64).reshape(-1)
    nthr, n = outcome.shape
    out = {}
    for idx, key in enumerate(WI_OUTCOMES):
        mask = outcome == idx
        if key in WI_PER_CLASS:
            arr = np.zeros((nthr, n_known, n))
            t, i = np.nonzero(mask)
            arr[t, lp[i] - 1, i] = 1.0
        else:
            arr = mask.astype(np.float64)
        out[key] = arr
    return out


class Plan(object):
    """Group-sorted arrays of one pass: `order` (N,) the original prediction row of each sorted position, `gt_order` (M,)
    the same for ground truths, pred_seg / gt_seg in sorted order and the (ngroups + 1) offsets."""

    def __init__(self, pred_seg, pred_group, gt_seg, gt_group, ngroups, rank=None):
        pred_group = np.asarray(pred_group, dtype=np.int64)
        gt_group = np.asarray(gt_group, dtype=np.int64)
        rows = np.arange(len(pred_group)) if rank is None else rank
        self.order = np.lexsort((rows, pred_group))
        self.gt_order = np.lexsort((np.arange(len(gt_group)), gt_group))
        self.pred_seg = np.ascontiguousarray(np.asarray(pred_seg, dtype=np.float64).reshape(-1, 2)[self.order])
        self.gt_seg = np.ascontiguousarray(np.asarray(gt_seg, dtype=np.float64).reshape(-1, 2)[self.gt_order])
        self.pred_start = self._starts(pred_group, ngroups)
        self.gt_start = self._starts(gt_group, ngroups)
        self.ngroups = ngroups
        self.device = None          # the uploaded copies, made once by match_device

    @staticmethod
    def _starts(group, ngroups):
        start = np.zeros(ngroups + 1, dtype=np.int64)
        np.cumsum(np.bincount(group, minlength=ngroups), out=start[1:])
        if start[-1] > np.iinfo(np.int32).max:
            raise ValueError("more than 2^31 - 1 rows")
        return start.astype(np.int32)

    def arrays(self):
        return self.pred_seg, self.pred_start, self.gt_seg, self.gt_start

    def unsort(self, codes):
        """(nthr, N) codes over sorted positions -> over the original prediction rows, ground-truth rows original too."""
        codes = np.where(codes >= 0, self.gt_order[np.maximum(codes, 0)], codes) if len(self.gt_order) else codes
        out = np.empty_like(codes)
        out[:, self.order] = codes
        return out


def video_codes(gt_video_ids, pred_video_ids):
    """Video names -> 0 .. nvid-1 in the order of sorted(set(names)).  -> (gt codes, prediction codes, nvid)."""
    names = np.concatenate([np.asarray(gt_video_ids, dtype=str), np.asarray(pred_video_ids, dtype=str)])
    uniq, inv = np.unique(names, return_inverse=True)
    inv = inv.reshape(-1)
    return inv[:len(gt_video_ids)], inv[len(gt_video_ids):], len(uniq)


def plan_split(prediction, ground_truth, codes=None):
    """The split pass (split_results_by_gt): group = video, in the order of sorted(set(videos)); file order inside."""
    gcode, pcode, nvid = codes if codes is not None else video_codes(ground_truth['video-id'], prediction['video-id'])
    return Plan(np.stack([prediction['t-start'], prediction['t-end']], 1), pcode,
                np.stack([ground_truth['t-start'], ground_truth['t-end']], 1), gcode, nvid)


def split_lists(plan, codes, prediction, ground_truth, nthr):
    """The three lists of split_results_by_gt from the codes of plan_split's groups (over sorted positions): sorted position
    order IS the CPU loop's order, video by video and in file order."""
    ood = prediction['ood_score'][plan.order]
    label = prediction['label'][plan.order]
    gt_label = ground_truth['label'][plan.gt_order]
    keys = ('bg', 'known', 'unknown')
    pred_scores = [{k: [] for k in keys} for _ in range(nthr)]
    pred_labels = [{k: [] for k in keys} for _ in range(nthr)]
    gt_labels = [{k: [] for k in keys} for _ in range(nthr)]
    for t in range(nthr):
        c = codes[t]
        matched = gt_label[np.maximum(c, 0)] if len(gt_label) else np.zeros(len(c), dtype=np.int64)
        masks = {'bg': c == -1, 'known': (c >= 0) & (matched != 0), 'unknown': (c >= 0) & (matched == 0)}
        for k, mask in masks.items():
            pred_scores[t][k] = ood[mask].tolist()
            pred_labels[t][k] = label[mask].tolist()
            gt_labels[t][k] = [-1.0] * int(mask.sum()) if k == 'bg' else matched[mask].tolist()
    return pred_scores, pred_labels, gt_labels


class APPlan(Plan):
    """The AP pass (compute_average_precision_detection, once per class): group = (class, video); inside a group the
    predictions follow the class's `score.argsort()[::-1]` -- the very expression of the CPU path, so both see the same
    permutation of equal scores.  class_rows[c] = the original prediction rows of class c in that order."""

    def __init__(self, prediction, ground_truth, classes, codes=None):
        gcode, pcode, nvid = codes if codes is not None else video_codes(ground_truth['video-id'], prediction['video-id'])
        classes = np.asarray(list(classes), dtype=np.int64)
        label, score = prediction['label'], prediction['score']
        by_label = np.argsort(label, kind='stable')
        lo = np.searchsorted(label[by_label], classes, side='left')
        hi = np.searchsorted(label[by_label], classes, side='right')
        rank = np.zeros(len(label), dtype=np.int64)
        self.class_rows = {}
        for c, a, b in zip(classes.tolist(), lo.tolist(), hi.tolist()):
            rows = by_label[a:b]                            # ascending rows: what a boolean mask selects
            rows = rows[score[rows].argsort()[::-1]]
            rank[rows] = np.arange(len(rows))
            self.class_rows[c] = rows
        counts = np.bincount(ground_truth['label'], minlength=int(classes.max()) + 1 if len(classes) else 0)
        self.gt_count = {c: int(counts[c]) for c in classes.tolist()}
        # groups that hold at least one row, numbered in (class, video) order
        keys = np.concatenate([ground_truth['label'] * nvid + gcode, label * nvid + pcode])
        uniq, inv = np.unique(keys, return_inverse=True)
        inv = inv.reshape(-1)
        m = len(gcode)
        Plan.__init__(self, np.stack([prediction['t-start'], prediction['t-end']], 1), inv[m:],
                      np.stack([ground_truth['t-start'], ground_truth['t-end']], 1), inv[:m], len(uniq), rank=rank)


def average_precision(plan, codes, classes, nthr, interpolated_prec_rec):
    """AP (nthr, len(classes)) from the codes of an APPlan (over ORIGINAL prediction rows, Plan.unsort), with the host
    arithmetic of compute_average_precision_detection in fp64: identical matches give identical numbers.  A class without
    ground truth raises KeyError like the CPU path."""
    classes = list(classes)
    ap = np.zeros((nthr, len(classes)))
    for c in classes:
        if plan.gt_count[c] == 0:
            raise KeyError(c)
        rows = plan.class_rows[c]
        if len(rows) == 0:
            continue                                        # ap[:, c - 1] stays 0, as the CPU path returns
        tp = (codes[:, rows] >= 0).astype(np.float64)
        fp = 1.0 - tp
        tp_cumsum = np.cumsum(tp, axis=1).astype(float)
        fp_cumsum = np.cumsum(fp, axis=1).astype(float)
        recall = tp_cumsum / float(plan.gt_count[c])
        precision = tp_cumsum / (tp_cumsum + fp_cumsum)
        for t in range(nthr):
            ap[t, c - 1] = interpolated_prec_rec(precision[t, :], recall[t, :])
    return ap


def _uploads(pred_seg, pred_start, gt_seg, gt_start, plan):
    """The four arrays on the current device: (pred_seg (N, 2), pred_start, gt_seg (M, 2), gt_start); made once per plan."""
    import torch
    dev = plan.device if plan is not None else None
    if dev is None:
        device = torch.device("cuda", torch.cuda.current_device())
        dev = tuple(torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(device)
                    for a, dt in ((pred_seg, np.float64), (pred_start, np.int32), (gt_seg, np.float64), (gt_start, np.int32)))
        dev = (dev[0].reshape(-1, 2), dev[1], dev[2].reshape(-1, 2), dev[3])
        if plan is not None:
            plan.device = dev
    return dev


def match_device(pred_seg, pred_start, gt_seg, gt_start, thresholds, plan=None):
    """match_reference through the kernel (ops.eval_match).  With `plan` (a Plan whose arrays the first four arguments
    are) the uploaded segments and offsets are kept on it and reused by later calls.  A result whose non-finite counter is
    non-zero is discarded: match_reference runs instead, with a warning (shown once per process by Python's default filter)."""
    import torch
    from ..common import ops
    thr = np.asarray(thresholds, dtype=np.float64).reshape(-1)
    if not 1 <= len(thr) <= MAX_THRESHOLDS:
        raise ValueError("1 .. %d tIoU thresholds, got %d" % (MAX_THRESHOLDS, len(thr)))
    dev = _uploads(pred_seg, pred_start, gt_seg, gt_start, plan)
    out, nonfinite = ops.eval_match(dev[0], dev[1], dev[2], dev[3], torch.from_numpy(thr).to(dev[0].device))
    result = out.cpu().numpy()              # the read-back waits for the kernel; the counter is final after it
    if int(nonfinite.item()) != 0:
        warnings.warn("eval_match: non-finite tIoU (zero-length segments) or a group with too many ground truths; "
                      "matching on the CPU instead")
        return match_reference(pred_seg, pred_start, gt_seg, gt_start, thr)
    return result


def match_labeled_device(pred_seg, pred_label, pred_start, gt_seg, gt_label, gt_start, thresholds, plan=None):
    """match_labeled_reference through the kernel (ops.eval_match_labeled), with match_device's conventions: the uploaded
    segments and offsets are kept on `plan` -- the very uploads match_device makes, so the split pass and this one share
    them; the labels are uploaded per call (set_ood_threshold changes them).  A result whose counter is non-zero is
    discarded for match_labeled_reference's, with a warning."""
    import torch
    from ..common import ops
    thr = np.asarray(thresholds, dtype=np.float64).reshape(-1)
    if not 1 <= len(thr) <= MAX_THRESHOLDS:
        raise ValueError("1 .. %d tIoU thresholds, got %d" % (MAX_THRESHOLDS, len(thr)))
    dev = _uploads(pred_seg, pred_start, gt_seg, gt_start, plan)
    labels = [torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32).reshape(-1)).to(dev[0].device) for a in (pred_label, gt_label)]
    out, top, nonfinite = ops.eval_match_labeled(dev[0], labels[0], dev[1], dev[2], labels[1], dev[3],
                                                 torch.from_numpy(thr).to(dev[0].device))
    result, max_tiou = out.cpu().numpy(), top.cpu().numpy()     # the read-back waits for the kernel; the counter is final
    if int(nonfinite.item()) != 0:
        warnings.warn("eval_match_labeled: non-finite tIoU (zero-length segments) or a group with too many ground truths; "
                      "matching on the CPU instead")
        return match_labeled_reference(pred_seg, pred_label, pred_start, gt_seg, gt_label, gt_start, thr)
    return result, max_tiou


def plan_ap(prediction, ground_truth, classes, codes=None):
    """The AP pass's planner: group = (class, video), order inside a group = the class's `argsort()[::-1]` rank."""
    return APPlan(prediction, ground_truth, classes, codes)
