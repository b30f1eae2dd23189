"""Wilderness Impact from detection tables: the WI pass of the open-set evaluation without proposal dicts, without a result
JSON and without the (nthr, K, N) outcome arrays of the host path.

table_ap.py is the step from a table to mAP and table_open.py the step to AUROC / AUPR / FAR@95 / OSDR; this module is the
step to the one open-set number that needs a known / unknown operating point, ANETdetection(openset=True) +
set_ood_threshold(thr) + evaluate('WI')[2]: the rule, stated once in numpy (`wi_reference`; `codes_reference` is its
arithmetic behind the matching), and the device path (`table_wi`: torch for the filter and the sort, ops.eval_match_labeled,
then ops.wilderness_impact -- csrc/wi.hip).

The rule is wrapper_compute_wilderness_impact + compute_wilderness_impact (eval_detection.py) with every free choice fixed.
Detections are the table's columns video int32 (N), cls int32 0-based (N), seg fp64 (N, 2), known fp64 (N); ground truths are
video, cls, seg in the same layout, cls = -1 marking a ground truth of a class outside the known ones.

  * detections of a video that has no ground-truth row at all are dropped first, and so are detections whose class is outside
    the index, as ANETdetection._import_prediction drops them;
  * a detection's label is cls + 1, or 0 ('__unknown__') where (1.0 - known) < ood_threshold in fp64 -- the expression of
    table_open.codes_reference and of ANETdetection.set_ood_threshold; a ground truth's label is cls + 1, or 0 for cls -1;
  * the pass order: a group is a video; the videos follow the evaluator's split plan (match.video_codes: np.unique over the
    names, that is ASCENDING VIDEO NAME), the detections of a video their table row, its ground truths their row.  WI is a
    sum over cumulative curves along this order, so it depends on it, and a driver numbers its videos by list position, not
    by name: `video_rank` (nvid,) carries the rank of each video number in the evaluator's order (None: the numbers are the
    ranks).  table_wi derives it from GroundTruth.video_index (`video_rank`), on the host, once per ground truth;
  * matching is match.match_labeled_reference over these groups (a ground truth is locked by a true positive only; equal
    tIoU goes to the lowest row) and the outcome of a row is match.wi_outcome_codes';
  * the arithmetic is compute_wilderness_impact's in its expression order.  With num_gt the float32 counts per label as the
    evaluator forms them (np.bincount(...).astype(np.float32); Kt = num_gt[1:].sum(), U = num_gt[0]) and cumulative sums
    along the pass order: recall ratio = Kt / (Kt + U - cumsum(tp_u2u)); for class c, over the rows whose detection has label
    c + 1, precision ratio = (tp + fp) / (tp + fp + fpu + 1e-6) with tp / fp / fpu the cumulative tp_k2k, fp_k2k + fp_bg2k and
    fp_u2k; WI[t, c] = utils_eval.interpolated_prec_rec(precision ratio, recall ratio).  Every ground-truth count and their
    total must be below 2^24, where the float32 counts stop being exact (asserted); a ground truth without any known row is
    refused with a ValueError (the recall ratio would be 0 / 0);
  * no detection at all gives 0: interpolated_prec_rec of empty curves is (1 - 0) * 0.

interpolated_prec_rec sums, over the rows where the recall ratio changes, the recall step times the precision envelope (the
maximum at or behind the row).  The recall ratio changes at row 0 (from the prepended 0 to Kt / (Kt + U - u_0) > 0) and at
every later tp_u2u row (Kt / (D - u) and Kt / (D - u + 1) differ by a relative 1 / D >> 2^-53 for D < 2^25); the closing step to
the appended 1 meets the appended precision 0 and adds +0.0.  otal_wilderness_impact sums exactly these terms in an order of
its own.

Tolerance.  Both sides form bit-identical terms: the same integer counts (exact in fp64), the same fp64 sums, quotients and
differences in the same operation order, one product per recall step; the library is built with -ffp-contract=off.  All terms
are >= 0.  Every precision ratio is below 1 and the computed recall ratios are monotone and at most 1 (rounding is monotone),
so with u = 2^-53 each computed term is at most (1 + u)^2 times its exact recall step and the exact sum S of the computed terms
is at most (1 + u)^2.  Only the order of adding the m terms differs, m = the tp_u2u rows + 1 <= the unknown ground truths + 1
(a tp_u2u locks its ground truth).  Any order of adding m non-negative terms errs by at most (m - 1) u S / (1 - (m - 1) u); the
two sides together differ by at most twice that, 2 (m - 1) 2^-53 (1 + 2^-25) for every m below 2^24.  `tolerance(m)` =
4 (m + 1) 2^-53 leaves a factor of two.

table_wi reads the tables' row counts (one host read per table) and nothing else before the final copy of the result; it
builds no (nthr, K, N) array and no outcome array: the kernel derives each row's outcome from its code and the two labels."""
import warnings

import numpy as np

from .match import MAX_THRESHOLDS, match_labeled_reference, wi_outcome_codes
from .utils_eval import interpolated_prec_rec

MAX_GT = 2 ** 24        # ops.WI_MAX_GT / OTAL_WI_MAX_GT: float32 counts are exact below it


def tolerance(m):
    """The bound on |kernel - wi_reference| per (threshold, class) for a sum of m terms, m = the tp_u2u detections + 1 <= the
    unknown ground truths + 1 (module docstring)."""
    return 4.0 * float(m + 1) * 2.0 ** -53


def video_rank(video_index):
    """{name: number} -> int64 (nvid,): the rank of each video number in the evaluator's order, ascending name
    (match.video_codes' np.unique)."""
    names = sorted(video_index, key=video_index.get)
    assert [video_index[n] for n in names] == list(range(len(names))), "video numbers are 0 .. nvid-1"
    rank = np.empty(len(names), dtype=np.int64)
    rank[np.argsort(np.asarray(names, dtype=str), kind='stable')] = np.arange(len(names))
    return rank


def gt_totals(gt_label, n_classes):
    """(Kt, U) as Python ints from the labels of ALL ground-truth rows, checked as the rule asks: num_gt as the evaluator
    forms it, every count and the total below 2^24, at least one known row."""
    num_gt = np.bincount(np.asarray(gt_label, dtype=np.int64).reshape(-1), minlength=n_classes + 1).astype(np.float32)
    assert (num_gt < MAX_GT).all() and float(num_gt.astype(np.float64).sum()) < MAX_GT, \
        "a ground-truth count at or above 2^24: the float32 counts of the rule are no longer exact"
    n_known, n_unknown = int(num_gt[1:].sum()), int(num_gt[0])
    if n_known == 0:
        raise ValueError("Wilderness Impact needs a ground truth of a known class: the recall ratio is 0 / 0 without one")
    return n_known, n_unknown


def codes_reference(codes, pred_label, gt_label, n_known, n_unknown, n_classes):
    """The arithmetic of the rule behind the matching; the oracle of otal_wilderness_impact.  codes (nthr, N) over the
    positions of the pass order (>= 0: the row of gt_label matched, -1 background, -2 nothing), pred_label (N) in 0 .. K,
    gt_label (M) in 0 .. K, n_known / n_unknown the ground-truth totals -> wi fp64 (nthr, K).  A code outside -2 .. M-1 or a
    label outside 0 .. K makes its row one without outcome, as the kernel treats it."""
    codes = np.asarray(codes, dtype=np.int64)
    codes = codes.reshape(codes.shape[0], -1)
    lp, lg = np.asarray(pred_label, dtype=np.int64).reshape(-1), np.asarray(gt_label, dtype=np.int64).reshape(-1)
    (nthr, N), M, K = codes.shape, len(lg), int(n_classes)
    in_range = (codes >= -2) & (codes < M) & ((lp >= 0) & (lp <= K))[None, :]
    safe = np.where(in_range, codes, -2)
    if M:
        matched_label = lg[np.maximum(safe, 0)]
        in_range &= (safe < 0) | ((matched_label >= 0) & (matched_label <= K))
    safe = np.where(in_range, safe, -2)
    outcome = wi_outcome_codes(safe, np.clip(lp, 0, K), np.clip(lg, 0, K))     # int8 (nthr, N), -1 for none
    kt, unknown = np.float32(n_known), np.float32(n_unknown)                    # num_gt[1:].sum(), num_gt[0]
    wi = np.zeros((nthr, K))
    tp_u2u_cumsum = np.cumsum((outcome == 0).astype(np.float64), axis=-1).astype(float)
    recall_ratio_cumsum = kt / (kt + unknown - tp_u2u_cumsum)
    for cidx in range(K):
        mine = (lp == cidx + 1)[None, :]
        tp_k2k_cumsum = np.cumsum(((outcome == 1) & mine).astype(np.float64), axis=-1).astype(float)
        fp_u2k_cumsum = np.cumsum(((outcome == 2) & mine).astype(np.float64), axis=-1).astype(float)
        fp_k2k_cumsum = np.cumsum((((outcome == 3) | (outcome == 6)) & mine).astype(np.float64), axis=-1).astype(float)
        precision_ratio_cumsum = (tp_k2k_cumsum + fp_k2k_cumsum) / (tp_k2k_cumsum + fp_k2k_cumsum + fp_u2k_cumsum + 1e-6)
        for tidx in range(nthr):
            wi[tidx, cidx] = interpolated_prec_rec(precision_ratio_cumsum[tidx, :], recall_ratio_cumsum[tidx, :])
    return wi


def labels_reference(cls, known, ood_threshold):
    """The detections' labels: cls + 1, 0 where the out-of-distribution score 1.0 - known is below ood_threshold."""
    label = np.asarray(cls, dtype=np.int64) + 1
    if ood_threshold is not None:
        label[(1.0 - np.asarray(known, dtype=np.float64)) < ood_threshold] = 0
    return label


def wi_reference(det, gt, thresholds, ood_threshold, n_classes=None, video_rank=None):
    """The rule (module docstring) in plain numpy.  det: video, cls, seg, known; gt: video, cls, seg -> wi fp64 (nthr, K).
    n_classes: the K of the class index (detections with cls outside 0 .. K-1 are dropped); None: the largest cls + 1.
    video_rank (nvid,): the rank of each video number in the evaluator's order; None: the numbers themselves."""
    thr = np.asarray(thresholds, dtype=np.float64).reshape(-1)
    gvideo, gcls, gseg = [np.asarray(gt[k]) for k in ('video', 'cls', 'seg')]
    video, cls, seg, known = [np.asarray(det[k]) for k in ('video', 'cls', 'seg', 'known')]
    gseg, seg = gseg.astype(np.float64).reshape(-1, 2), seg.astype(np.float64).reshape(-1, 2)
    K = int(n_classes) if n_classes is not None else max(int(max(cls.max(initial=-1), gcls.max(initial=-1))) + 1, 1)
    gvideo, glabel = gvideo.astype(np.int64), np.where(gcls >= 0, gcls.astype(np.int64) + 1, 0)
    n_known, n_unknown = gt_totals(glabel, K)
    keep = np.isin(video, np.unique(gvideo)) & (cls >= 0) & (cls < K)
    video, seg = video[keep].astype(np.int64), seg[keep]
    label = labels_reference(cls[keep], known[keep], ood_threshold)
    nvid = int(max(video.max(initial=-1), gvideo.max(initial=-1))) + 1
    rank = np.arange(nvid) if video_rank is None else np.asarray(video_rank, dtype=np.int64)
    group, ggroup = rank[video], rank[gvideo]
    ngroups = int(max(group.max(initial=-1), ggroup.max(initial=-1))) + 1
    order = np.argsort(group, kind='stable')                # (video rank, table row)
    gorder = np.argsort(ggroup, kind='stable')
    edges = np.arange(ngroups + 1)
    pred_start = np.searchsorted(group[order], edges).astype(np.int32)
    gt_start = np.searchsorted(ggroup[gorder], edges).astype(np.int32)
    codes, _ = match_labeled_reference(seg[order], label[order], pred_start, gseg[gorder], glabel[gorder], gt_start, thr)
    return codes_reference(codes, label[order], glabel[gorder], n_known, n_unknown, K)


def _host_columns(tables):
    from .table_open import _host_columns as columns
    return columns(tables)


def _gt_arrays(gt, device):
    """The ground truth in the pass order, uploaded once per GroundTruth and device: rank (nvid) int64 and has_gt (nvid) bool
    over video numbers; gt_seg (M, 2) fp64 and gt_label (M) int32, ALL rows sorted by (video rank, row); gt_start (nvid + 2)
    int32, their offsets per rank (the further group nvid, for the dropped detections, is empty); the two totals."""
    import torch
    cached = getattr(gt, '_wi', None)
    if cached is None or cached[0] != device:
        nvid = gt.nvid
        rank = video_rank(gt.video_index)
        label = np.where(gt.cls >= 0, gt.cls.astype(np.int64) + 1, 0)
        n_known, n_unknown = gt_totals(label, gt.n_classes)
        has_gt = np.zeros(max(nvid, 1), dtype=bool)
        has_gt[gt.video] = True
        group = rank[gt.video]
        order = np.argsort(group, kind='stable')
        gt_start = np.searchsorted(group[order], np.arange(nvid + 2)).astype(np.int32)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
        cached = (device, dict(rank=up(rank if nvid else np.zeros(1, dtype=np.int64)), has_gt=up(has_gt),
                               gt_seg=up(gt.seg[order]).reshape(-1, 2), gt_label=up(label[order].astype(np.int32)),
                               gt_start=up(gt_start), n_known=n_known, n_unknown=n_unknown))
        gt._wi = cached
    return cached[1]


def table_wi_counted(tables, gt, thresholds, ood_threshold):
    """table_wi without the fallback: (wi (nthr, K) of the kernel, the matching's non-finite counter).  A non-zero counter
    says that the array is to be discarded."""
    import torch
    from ..common import ops
    thr = np.asarray(thresholds, dtype=np.float64).reshape(-1)
    if not 1 <= len(thr) <= MAX_THRESHOLDS:
        raise ValueError("1 .. %d tIoU thresholds, got %d" % (MAX_THRESHOLDS, len(thr)))
    K, nvid, nthr = gt.n_classes, gt.nvid, len(thr)
    gt_totals(np.where(gt.cls >= 0, gt.cls.astype(np.int64) + 1, 0), K)     # the refusals, before any device work
    tables = list(tables)
    counts = [int(t['n']) for t in tables]              # the one host read per table
    if sum(counts) == 0:
        return np.zeros((nthr, K)), 0
    if sum(counts) > ops.AP_MAX_CLASS_ROWS:
        raise ValueError("more than %d detections" % ops.AP_MAX_CLASS_ROWS)
    device = tables[0]['video'].device
    dev = _gt_arrays(gt, device)
    cat = lambda k: torch.cat([t[k][:n] for t, n in zip(tables, counts)])
    video, cls, seg, known = cat('video').long(), cat('cls').long(), cat('seg'), cat('known')
    # a detection of a video without ground truth (or outside the index) moves to the further group nvid, which has no
    # ground truth, and takes the label -1, which has no outcome: no row count changes
    inside = (video >= 0) & (video < nvid) & (cls >= 0) & (cls < K)
    safe_video = video.clamp(0, max(nvid - 1, 0))
    keep = inside & dev['has_gt'][safe_video]
    label = cls + 1
    if ood_threshold is not None:
        label = torch.where((1.0 - known) < float(ood_threshold), torch.zeros_like(label), label)
    label = torch.where(keep, label, torch.full_like(label, -1)).int()
    group = torch.where(keep, dev['rank'][safe_video], torch.full_like(video, nvid))
    by_group = torch.sort(group, stable=True).indices               # (video rank, table row)
    pred_start = torch.searchsorted(group[by_group], torch.arange(nvid + 2, device=device)).int()
    pred_label = label[by_group].contiguous()
    codes, _, nonfinite = ops.eval_match_labeled(seg[by_group].contiguous(), pred_label, pred_start, dev['gt_seg'],
                                                 dev['gt_label'], dev['gt_start'], torch.from_numpy(thr).to(device))
    wi = ops.wilderness_impact(codes, pred_label, dev['gt_label'], dev['n_known'], dev['n_unknown'], K).cpu().numpy()
    # final: the read-back above waited for both kernels
    return wi, int(nonfinite.item())


def table_wi(tables, gt, thresholds, ood_threshold):
    """wi fp64 (nthr, K) on the host, of the detections of `tables` (a list of device tables of ops.detection_table, their
    `video` columns numbered by gt.video_index) against `gt` (a table_ap.GroundTruth) at the tIoU `thresholds`, detections
    with 1.0 - known below `ood_threshold` relabelled unknown: the rule of wi_reference through otal_eval_match_labeled and
    otal_wilderness_impact.  A non-zero non-finite counter of the matching (a zero-length detection on a zero-length ground
    truth, or a video of more than OTAL_EVAL_MAX_GT ground truths) gives wi_reference's result instead, with a warning."""
    tables = list(tables)
    wi, counter = table_wi_counted(tables, gt, thresholds, ood_threshold)
    if counter != 0:
        warnings.warn("table_wi: non-finite tIoU (zero-length segments) or a video with too many ground truths; "
                      "evaluating on the CPU instead")
        return wi_reference(_host_columns(tables), gt.columns(), thresholds, ood_threshold, n_classes=gt.n_classes,
                            video_rank=video_rank(gt.video_index))
    return wi
