"""AUROC, AUPR, FAR@95 and OSDR from detection tables: the open-set numbers of the evaluation without proposal dicts and
without a result JSON.

table_ap.py is the step from a table to mAP; this module is the step from a table to the four open-set numbers that
compute_auc_scores and compute_osdr_scores (eval_detection.py) give per tIoU threshold: the rule, stated once in numpy
(`open_reference`), and the device path (`table_open`: torch for the sorts and offsets, ops.eval_match with group = video, a
scatter of the matched detections into one slot per ground truth, then ops.open_set_curves -- csrc/oscurve.hip).

The rule is split_results_by_gt + compute_auc_scores + compute_osdr_scores with every free choice fixed.  Detections are the
table's columns video int32 (N), cls int32 0-based (N), seg fp64 (N, 2), known fp64 (N); ground truths are video, cls, seg in
the same layout, cls = -1 marking a ground truth of a class outside the known ones.

  * detections of a video that has no ground-truth row at all are dropped first, and so are detections whose class is outside
    the index, as ANETdetection._import_prediction drops them;
  * the split pass: a group is a video, its detections in table row order (the order of the result file), its ground truths
    all rows of that video, the unknown ones included, in their order; match.match_reference gives the codes;
  * the foreground of a threshold is the rows with code >= 0.  For such a row, unknown = the matched ground truth has cls -1,
    ood = 1.0 - known in fp64, the predicted label is cls -- or "unknown" where an ood_threshold is given and ood <
    ood_threshold (ANETdetection.set_ood_threshold) -- and correct = not unknown and predicted label == the ground truth's cls;
  * AUPR = utils_eval.average_precision_score and AUROC = utils_eval.roc_auc_score of (unknown, ood), unknown the positive
    kind, in fp64 (the host functions store float32); AUROC is 0 when only one kind is present;
  * FAR@95 = fpr[argmin |tpr - 0.95|] on utils_eval.roc_curve WITH drop_intermediate, as the host computes it: twenty tied
    (unknown, known) pairs give tpr_j = fpr_j = j / 20, of which the full curve would pick j = 19 (0.95) and the curve without
    its equal-step interior points keeps j = 1 and j = 20 and picks 1.0.  No unknown matched: 0 (argmin over NaN is 0 and
    fpr[0] = 0); no known matched: NaN;
  * OSDR = utils_eval.open_set_detection_rate with confidence = known.  The order is ascending known, equal values by
    ascending table row (the host's unstable argsort leaves them to the numpy build).  Both coordinates of the cuts are
    non-increasing in the cut index, so the host's lexsort of the curve points is the cut order itself -- (1, 1), cut 0 ..
    cut n-2, (0, 0) -- and the area is the trapezoid sum over that order, with no second sort; n = 1 gives 0.5;
  * an empty foreground gives 0 for all four (the host leaves its zero-initialised arrays).

Tolerance.  The kernel forms exactly the terms of the rule: the same integer counts (tps, fps, suffix counts) and the same
fp64 quotients, differences and products in the same operation order -- (recall - previous recall) * precision is the exact
negation of numpy's diff(recall) * precision.  Each of AUROC, AUPR and OSDR is a sum of m <= n + 1 such terms, all >= 0, whose
exact sum S is at most 1 + 3 * 2^-53.  Any order of adding m non-negative terms errs by at most (m - 1) 2^-53 S / (1 - (m - 1)
2^-53); the two sides together differ by at most twice that, under 2 (n + 1) 2^-53 (1 + 2^-40) for every n that fits an int32.
`tolerance(n)` = 4 (n + 2) 2^-53 leaves a factor of two.  FAR@95 is a quotient of two integers that both sides pick by comparing
identical fp64 expressions (|tps / P - 0.95|, the first smallest): it is bit-equal, NaN for NaN.

table_open reads the tables' row counts (one host read per table) and nothing else before the final copy of the result: a
ground truth is taken at most once per threshold, so the M ground-truth rows bound every threshold's foreground and the
scatter needs no count from the device."""
import warnings

import numpy as np

from .match import MAX_THRESHOLDS, match_reference
from .utils_eval import average_precision_score, roc_auc_score, roc_curve

KEYS = ('auroc', 'aupr', 'far95', 'osdr')       # the columns of otal_open_set_curves' result


def tolerance(n):
    """The bound on |kernel - open_reference| for AUROC, AUPR and OSDR over a foreground of n rows (module docstring)."""
    return 4.0 * float(n + 2) * 2.0 ** -53


def osdr_reference(known, row, correct, unknown):
    """The OSDR of one foreground: ascending (known, row), the trapezoid sum over (1, 1), the cuts, (0, 0)."""
    n = len(known)
    if n == 0:
        return 0.0
    order = np.lexsort((row, known))
    s_k, s_u = correct[order].astype(np.float64), unknown[order].astype(np.float64)
    P = int(unknown.sum())
    Q = n - P
    # cut k (k = 0 .. n-2): correct knowns strictly behind it, unknowns at or behind it
    suffix_k = np.concatenate((np.cumsum(s_k[::-1])[::-1], [0.0]))
    suffix_u = np.cumsum(s_u[::-1])[::-1]
    ccr = suffix_k[1:n] / float(Q) if Q > 0 else np.ones(n - 1)
    fpr = suffix_u[:n - 1] / float(P) if P > 0 else np.zeros(n - 1)
    f, c = np.concatenate(([1.0], fpr, [0.0])), np.concatenate(([1.0], ccr, [0.0]))
    return float(np.sum((f[:-1] - f[1:]) * (c[:-1] + c[1:]) / 2.0))


def curves_reference(known, row, correct, unknown):
    """(AUROC, AUPR, FAR@95, OSDR) of one foreground in fp64: known (n) fp64, row (n) the table rows, correct / unknown (n)
    bool.  The arithmetic of the rule behind the matching; the oracle of otal_open_set_curves."""
    n = len(known)
    if n == 0:
        return 0.0, 0.0, 0.0, 0.0
    known = np.asarray(known, dtype=np.float64)
    unknown = np.asarray(unknown, dtype=bool)
    correct = np.asarray(correct, dtype=bool) & ~unknown
    ood = 1.0 - known
    labels = unknown.astype(np.int64)
    aupr = average_precision_score(labels, ood)
    auroc = roc_auc_score(labels, ood) if 0 < int(unknown.sum()) < n else 0.0
    fpr, tpr, _ = roc_curve(labels, ood)
    far = float(fpr[np.abs(tpr - 0.95).argmin()])
    return auroc, aupr, far, osdr_reference(known, np.asarray(row), correct, unknown)


def codes_reference(codes, row, known, cls, gt_cls, ood_threshold=None):
    """The rule behind the matching: codes (nthr, N) over group-sorted positions (>= 0: the row of gt_cls taken), row (N) the
    table row of a position, known / cls over table rows, gt_cls (M) with -1 for unknown -> fp64 (nthr, 4) in KEYS' order."""
    codes, row, known, cls, gt_cls = (np.asarray(a) for a in (codes, row, known, cls, gt_cls))
    out = np.zeros((codes.shape[0], 4))
    for t in range(codes.shape[0]):
        fg = np.nonzero(codes[t] >= 0)[0]
        r = row[fg]
        g = gt_cls[codes[t, fg]]
        pred = cls[r].copy()
        if ood_threshold is not None:
            pred[(1.0 - known[r]) < ood_threshold] = -1
        out[t] = curves_reference(known[r], r, pred == g, g == -1)
    return out


def open_reference(det, gt, thresholds, ood_threshold=None, n_classes=None):
    """The rule (module docstring) in plain numpy.  det: video, cls, seg, known; gt: video, cls, seg -> dict(auroc, aupr,
    far95, osdr), each fp64 (nthr,).  n_classes: the K of the class index (detections with cls outside 0 .. K-1 are dropped);
    None: every cls >= 0 is inside it."""
    thr = np.asarray(thresholds, dtype=np.float64).reshape(-1)
    gvideo, gcls, gseg = [np.asarray(gt[k]) for k in ('video', 'cls', 'seg')]
    video, cls, seg, known = [np.asarray(det[k]) for k in ('video', 'cls', 'seg', 'known')]
    gseg, seg = gseg.astype(np.float64).reshape(-1, 2), seg.astype(np.float64).reshape(-1, 2)
    keep = np.isin(video, np.unique(gvideo)) & (cls >= 0)
    if n_classes is not None:
        keep &= cls < n_classes
    video, cls, seg, known = video[keep].astype(np.int64), cls[keep].astype(np.int64), seg[keep], known[keep].astype(np.float64)
    gvideo, gcls = gvideo.astype(np.int64), gcls.astype(np.int64)
    nvid = int(max(video.max(initial=-1), gvideo.max(initial=-1))) + 1
    order = np.argsort(video, kind='stable')                # (video, table row)
    gorder = np.argsort(gvideo, kind='stable')
    edges = np.arange(nvid + 1)
    pred_start = np.searchsorted(video[order], edges).astype(np.int32)
    gt_start = np.searchsorted(gvideo[gorder], edges).astype(np.int32)
    codes = match_reference(seg[order], pred_start, gseg[gorder], gt_start, thr)
    res = codes_reference(codes, order, known, cls, gcls[gorder], ood_threshold)
    return {k: res[:, i].copy() for i, k in enumerate(KEYS)}


def _host_columns(tables):
    """The first n rows of the tables as open_reference's detection columns, on the host."""
    parts = [{k: t[k][:int(t['n'])].cpu().numpy() for k in ('video', 'cls', 'seg', 'known')} for t in tables]
    cat = lambda k, shape, dt: np.concatenate([p[k] for p in parts]) if parts else np.zeros(shape, dtype=dt)
    return dict(video=cat('video', 0, np.int32), cls=cat('cls', 0, np.int32), seg=cat('seg', (0, 2), np.float64),
                known=cat('known', 0, np.float64))


def table_open_counted(tables, gt, thresholds, ood_threshold=None):
    """table_open without the fallback: (dict(auroc, aupr, far95, osdr) of the kernels, the matching's non-finite counter).
    A non-zero counter says that the dict is to be discarded."""
    import torch
    from ..common import ops
    thr = np.asarray(thresholds, dtype=np.float64).reshape(-1)
    if not 1 <= len(thr) <= MAX_THRESHOLDS:
        raise ValueError("1 .. %d tIoU thresholds, got %d" % (MAX_THRESHOLDS, len(thr)))
    K, nvid, nthr = gt.n_classes, gt.nvid, len(thr)
    tables = list(tables)
    counts = [int(t['n']) for t in tables]              # the one host read per table
    M = len(gt.video)
    if sum(counts) == 0 or M == 0:
        return {k: np.zeros(nthr) for k in KEYS}, 0
    if sum(counts) > ops.AP_MAX_CLASS_ROWS:
        raise ValueError("more than %d detections" % ops.AP_MAX_CLASS_ROWS)
    device = tables[0]['video'].device
    dev = gt.split_arrays(device)
    cat = lambda k: torch.cat([t[k][:n] for t, n in zip(tables, counts)])
    video, cls, seg, known = cat('video').long(), cat('cls').long(), cat('seg'), cat('known')
    N = video.numel()
    # a detection of a video without ground truth (or outside the index) moves to the further group nvid, which has no
    # ground truth: it matches nothing and no row count changes
    inside = (video >= 0) & (video < nvid) & (cls >= 0) & (cls < K)
    keep = inside & dev['has_gt'][video.clamp(0, max(nvid - 1, 0))]
    group = torch.where(keep, video, torch.full_like(video, nvid))
    by_group = torch.sort(group, stable=True).indices               # (video, table row)
    pred_start = torch.searchsorted(group[by_group], torch.arange(nvid + 2, device=device)).int()
    codes, nonfinite = ops.eval_match(seg[by_group].contiguous(), pred_start, dev['gt_seg'], dev['gt_start'],
                                      torch.from_numpy(thr).to(device))
    res = codes_to_curves(codes, by_group, known, cls, dev['gt_cls'], ood_threshold).cpu().numpy()
    # final: the read-back above waited for both kernels
    return {k: res[:, i].copy() for i, k in enumerate(KEYS)}, int(nonfinite.item())


def codes_to_curves(codes, by_group, known, cls, gt_cls, ood_threshold=None):
    """codes_reference on the device, without a host read: codes (nthr, N) int32 of eval_match, by_group (N) int64 the table
    row of a position, known (rows) fp64, cls (rows) int64, gt_cls (M) int32 -> (nthr, 4) fp64 on the device.  A ground truth
    is taken at most once per threshold, so the matched detections of a threshold fit its M slots."""
    import torch
    from ..common import ops
    device = codes.device
    (nthr, N), M = codes.shape, gt_cls.numel()
    if N == 0 or M == 0:
        return torch.zeros((nthr, 4), dtype=torch.float64, device=device)
    # one slot per (threshold, ground truth): the group-sorted position of the detection that took it, -1 for none.  The
    # rows without a match all write -1 into a spare column.
    hit = codes >= 0
    position = torch.arange(N, device=device).expand(nthr, N)
    slot = torch.full((nthr, M + 1), -1, dtype=torch.int64, device=device)
    slot.scatter_(1, torch.where(hit, codes.long(), torch.full_like(position, M)),
                  torch.where(hit, position, torch.full_like(position, -1)))
    slot = slot[:, :M]
    filled = slot >= 0
    row = by_group[slot.clamp(min=0)]                               # (nthr, M): the table row of a slot's detection
    kn = known[row]
    gcls = gt_cls.long().expand(nthr, M)
    unknown = gcls < 0
    correct = (cls[row] == gcls) & ~unknown
    if ood_threshold is not None:
        correct &= ~((1.0 - kn) < float(ood_threshold))
    flags = torch.where(filled, unknown.int() + 2 * correct.int(), torch.full((), -1, dtype=torch.int32, device=device))
    # stable sorts from the last key to the first: table row, then known, then the empty slots behind the others
    order = torch.sort(torch.where(filled, row, torch.full_like(row, N)), dim=1, stable=True).indices
    order = order.gather(1, torch.sort(kn.gather(1, order), dim=1, stable=True).indices)
    order = order.gather(1, torch.sort((~filled).gather(1, order).to(torch.uint8), dim=1, stable=True).indices)
    return ops.open_set_curves(kn.gather(1, order).contiguous(), flags.gather(1, order).contiguous())


def table_open(tables, gt, thresholds, ood_threshold=None):
    """dict(auroc, aupr, far95, osdr) of fp64 (nthr,) on the host, of the detections of `tables` (a list of device tables of
    ops.detection_table, their `video` columns numbered by gt.video_index) against `gt` (a table_ap.GroundTruth) at the tIoU
    `thresholds`: the rule of open_reference through otal_eval_match and otal_open_set_curves.  A non-zero non-finite counter of
    the matching (a zero-length detection on a zero-length ground truth, or a video of more than OTAL_EVAL_MAX_GT ground truths)
    gives open_reference's result instead, with a warning."""
    tables = list(tables)
    result, counter = table_open_counted(tables, gt, thresholds, ood_threshold)
    if counter != 0:
        warnings.warn("table_open: non-finite tIoU (zero-length segments) or a video with too many ground truths; "
                      "evaluating on the CPU instead")
        return open_reference(_host_columns(tables), gt.columns(), thresholds, ood_threshold, n_classes=gt.n_classes)
    return result
