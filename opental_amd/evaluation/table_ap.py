"""Average precision from detection tables: the AP pass of the evaluation without proposal dicts and without a result JSON.

The inference pipelines leave the Soft-NMS rows on the device and otal_detection_table (common/det_table.py) turns them into
one compact table; otal_eval_match (match.py) does the greedy matching.  This module is the step between a table and a
number: the rule, stated once in numpy (`ap_reference`), the ground truth as column arrays (`GroundTruth`) and the device
path (`table_ap`: torch for the sorts and offsets, ops.eval_match, then ops.average_precision -- csrc/ap.hip).

The rule is compute_average_precision_detection (eval_detection.py) with every free choice fixed.  Detections are columns
video int32 (N), cls int32 0-based (N), seg fp64 (N, 2), score fp32 (N) -- a table's columns with score = sup[:, 0]; ground
truths are video, cls, seg in the same layout, cls = -1 marking a ground truth of a class outside the known ones.

  * detections of a video that has no ground-truth row at all are dropped first, as ANETdetection._import_prediction drops
    them; a row with cls = -1 counts as a ground-truth row for this test (and for nothing else);
  * inside a class the detections are visited by descending score, equal scores by ascending table row (the host path's
    `argsort()[::-1]` leaves equal scores to the numpy build);
  * matching is match.match_reference over the groups (class, video), a group's detections in that order;
  * with tp_cum the running count of matched detections, precision = tp_cum / (position + 1) and recall = tp_cum / npos in
    fp64, npos the class's ground truths; AP = utils_eval.interpolated_prec_rec(precision, recall);
  * a class without detections has AP 0; a class without ground truth raises KeyError(c + 1), as the host path does.

interpolated_prec_rec sums, over the positions where the recall changes -- the matched detections -- the recall step times
the precision envelope (the maximum over the later positions); the appended recall 1.0 meets the appended precision 0 and
adds nothing.  The kernel sums exactly these terms, tp_cum / npos - (tp_cum - 1) / npos times the envelope, in an order of its
own.  Both sides hold the same integer counts and the same fp64 quotients; they differ in the order of adding at most npos
terms of at most 1 / npos each (relative rounding 2^-53 per addition) and in the cancellation of the recall step (2^-53
absolute per term), so |AP_device - AP_reference| <= 4 npos 2^-53: `tolerance`.

Groups are numbered densely, class * nvid + video with one further class K for the dropped rows, and the offsets include the
empty groups: otal_eval_match leaves a group without detections at once, and no count has to come back to the host to size
an array.  table_ap reads the tables' row counts (one host read per table) and nothing else before the final copy of the
result."""
import json
import warnings

import numpy as np

from .match import MAX_THRESHOLDS, match_reference
from .utils_eval import interpolated_prec_rec


def tolerance(npos):
    """The bound on |AP of the kernel - AP of ap_reference| for a class of npos ground truths (module docstring)."""
    return 4.0 * float(npos) * 2.0 ** -53


def _columns(table, keys):
    return [np.asarray(table[k]) for k in keys]


def class_order(cls, score):
    """The rows in (cls, descending score, row) order."""
    return np.lexsort((np.arange(len(cls)), -np.asarray(score, dtype=np.float64), cls))


def ap_reference(det, gt, thresholds, n_classes):
    """The rule (module docstring) in plain numpy.  det: video, cls, seg, score; gt: video, cls, seg -> ap fp64
    (nthr, n_classes)."""
    thr = np.asarray(thresholds, dtype=np.float64).reshape(-1)
    gvideo, gcls, gseg = _columns(gt, ('video', 'cls', 'seg'))
    video, cls, seg, score = _columns(det, ('video', 'cls', 'seg', 'score'))
    gseg, seg = gseg.astype(np.float64).reshape(-1, 2), seg.astype(np.float64).reshape(-1, 2)
    gt_count = np.bincount(gcls[gcls >= 0], minlength=n_classes)
    for c in range(n_classes):
        if gt_count[c] == 0:
            raise KeyError(c + 1)
    keep = np.isin(video, np.unique(gvideo)) & (cls >= 0) & (cls < n_classes)
    video, cls, seg, score = video[keep].astype(np.int64), cls[keep].astype(np.int64), seg[keep], score[keep]
    known = gcls >= 0
    gvideo, gcls, gseg = gvideo[known].astype(np.int64), gcls[known].astype(np.int64), gseg[known]
    nvid = int(max(video.max(initial=-1), gvideo.max(initial=-1))) + 1
    by_class = class_order(cls, score)                      # the r-th row in (class, rank) order
    key, gkey = cls * nvid + video, gcls * nvid + gvideo
    # stable over the class order: (class, video, rank)
    by_group = by_class[np.argsort(key[by_class], kind='stable')]
    gorder = np.argsort(gkey, kind='stable')
    edges = np.arange(n_classes * nvid + 1)
    pred_start = np.searchsorted(key[by_group], edges).astype(np.int32)
    gt_start = np.searchsorted(gkey[gorder], edges).astype(np.int32)
    codes = match_reference(seg[by_group], pred_start, gseg[gorder], gt_start, thr)
    position = np.empty(len(by_group), dtype=np.int64)      # the group-sorted position of every row
    position[by_group] = np.arange(len(by_group))
    rank_pos = position[by_class]
    class_start = np.searchsorted(cls[by_class], np.arange(n_classes + 1))
    ap = np.zeros((len(thr), n_classes))
    for c in range(n_classes):
        rows = rank_pos[class_start[c]:class_start[c + 1]]
        if len(rows) == 0:
            continue
        tp_cum = np.cumsum(codes[:, rows] >= 0, axis=1).astype(np.float64)
        precision = tp_cum / np.arange(1, len(rows) + 1, dtype=np.float64)
        recall = tp_cum / float(gt_count[c])
        for t in range(len(thr)):
            ap[t, c] = interpolated_prec_rec(precision[t], recall[t])
    return ap


def class_names(cls_idx_detection, dataset='thumos14'):
    """The known classes of a class index file in its order, as ANETdetection.get_activity_index reads it: the second word of
    a line for THUMOS14, the whole line for ActivityNet."""
    with open(cls_idx_detection, 'r') as f:
        lines = [l for l in f.read().splitlines() if l.strip()]
    return [l.split()[1] if dataset in ('thumos14', 'thumos_anet') else l.strip() for l in lines]


class GroundTruth(object):
    """The column arrays of an ANETdetection-style ground-truth JSON: video int32 (M), cls int32 (M; -1 for a label outside
    the class index), seg fp64 (M, 2), one row per annotation of every video of the requested subsets, in file order
    (ANETdetection._import_ground_truth).  `video_index` maps a video's name to its number: the names of `videos` first, in
    their order (a driver numbers its test videos 0 .. V-1 this way, whether they have ground truth or not), then the
    remaining videos of the file in their order."""

    def __init__(self, video, cls, seg, n_classes, video_index):
        self.video = np.ascontiguousarray(video, dtype=np.int32).reshape(-1)
        self.cls = np.ascontiguousarray(cls, dtype=np.int32).reshape(-1)
        self.seg = np.ascontiguousarray(seg, dtype=np.float64).reshape(-1, 2)
        self.n_classes = int(n_classes)
        self.video_index = dict(video_index)
        self.gt_count = np.bincount(self.cls[self.cls >= 0], minlength=self.n_classes).astype(np.int32)
        self._device = None
        self._split = None

    @classmethod
    def load(cls, ground_truth_filename, cls_idx_detection, subset=('validation',), dataset='thumos14', videos=None):
        with open(ground_truth_filename, 'r') as fobj:
            data = json.load(fobj)
        if 'database' not in data:
            raise IOError('Please input a valid ground truth file.')
        class_to_idx = {name: i for i, name in enumerate(class_names(cls_idx_detection, dataset))}
        rows = [(vid, ann) for vid, v in data['database'].items() if v['subset'] in subset for ann in v['annotations']]
        video_index = {}
        for name in list(videos or []) + [vid for vid, _ in rows]:
            video_index.setdefault(name, len(video_index))
        return cls([video_index[vid] for vid, _ in rows], [class_to_idx.get(ann['label'], -1) for _, ann in rows],
                   [ann['segment'][:2] for _, ann in rows], len(class_to_idx), video_index)

    @property
    def nvid(self):
        return len(self.video_index)

    def columns(self):
        return dict(video=self.video, cls=self.cls, seg=self.seg)

    def device_arrays(self, device):
        """The arrays table_ap needs, uploaded once: has_gt (nvid) bool; gt_seg (M', 2) fp64, the rows of the known classes
        sorted by (class, video, row); gt_start ((K + 1) * nvid + 1) int32, their offsets per group class * nvid + video
        (the groups of the further class K are empty); gt_count (K) int32."""
        import torch
        if self._device is None or self._device[0] != device:
            K, nvid = self.n_classes, self.nvid
            if (K + 1) * nvid + 1 > np.iinfo(np.int32).max:
                raise ValueError("more than 2^31 - 1 (class, video) groups")
            has_gt = np.zeros(max(nvid, 1), dtype=bool)
            has_gt[self.video] = True
            known = self.cls >= 0
            key = self.cls[known].astype(np.int64) * nvid + self.video[known]
            order = np.argsort(key, kind='stable')
            gt_start = np.searchsorted(key[order], np.arange((K + 1) * nvid + 1)).astype(np.int32)
            seg = np.ascontiguousarray(self.seg[known][order])
            up = lambda a: torch.from_numpy(a).to(device)
            self._device = (device, dict(has_gt=up(has_gt), gt_seg=up(seg).reshape(-1, 2), gt_start=up(gt_start),
                                         gt_count=up(self.gt_count)))
        return self._device[1]

    def split_arrays(self, device):
        """The arrays of the split pass (table_open), uploaded once: has_gt (nvid) bool; gt_seg (M, 2) fp64 and gt_cls (M)
        int32, ALL rows, the unknown ones (cls = -1) included, sorted by (video, row); gt_start (nvid + 2) int32, their offsets
        per video (the further group nvid, for the dropped detections, is empty)."""
        import torch
        if self._split is None or self._split[0] != device:
            nvid = self.nvid
            has_gt = np.zeros(max(nvid, 1), dtype=bool)
            has_gt[self.video] = True
            order = np.argsort(self.video, kind='stable')
            gt_start = np.searchsorted(self.video[order], np.arange(nvid + 2)).astype(np.int32)
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
            self._split = (device, dict(has_gt=up(has_gt), gt_seg=up(self.seg[order]).reshape(-1, 2),
                                        gt_cls=up(self.cls[order]), gt_start=up(gt_start)))
        return self._split[1]


def _host_columns(tables):
    """The first n rows of the tables as ap_reference's detection columns, on the host."""
    parts = [{k: t[k][:int(t['n'])].cpu().numpy() for k in ('video', 'cls', 'seg', 'sup')} for t in tables]
    cat = lambda k, shape, dt: np.concatenate([p[k] for p in parts]) if parts else np.zeros(shape, dtype=dt)
    return dict(video=cat('video', 0, np.int32), cls=cat('cls', 0, np.int32), seg=cat('seg', (0, 2), np.float64),
                score=cat('sup', (0, 3), np.float32)[:, 0])


def table_ap(tables, gt, thresholds):
    """ap fp64 (nthr, K) on the host, of the detections of `tables` (a list of device tables of ops.detection_table, their
    `video` columns numbered by gt.video_index) against `gt` (a GroundTruth) at the tIoU `thresholds`: the rule of
    ap_reference through otal_eval_match and otal_average_precision.  A non-zero non-finite counter of the matching (a
    zero-length detection on a zero-length ground truth, or a group of more than OTAL_EVAL_MAX_GT ground truths) gives
    ap_reference's result instead, with a warning."""
    import torch
    from ..common import ops
    thr = np.asarray(thresholds, dtype=np.float64).reshape(-1)
    if not 1 <= len(thr) <= MAX_THRESHOLDS:
        raise ValueError("1 .. %d tIoU thresholds, got %d" % (MAX_THRESHOLDS, len(thr)))
    K, nvid = gt.n_classes, gt.nvid
    for c in range(K):
        if gt.gt_count[c] == 0:
            raise KeyError(c + 1)
    tables = list(tables)
    if not tables:
        return np.zeros((len(thr), K))
    device = tables[0]['video'].device
    dev = gt.device_arrays(device)
    counts = [int(t['n']) for t in tables]              # the one host read per table
    if sum(counts) > ops.AP_MAX_CLASS_ROWS:
        raise ValueError("more than %d detections" % ops.AP_MAX_CLASS_ROWS)
    cat = lambda k: torch.cat([t[k][:n] for t, n in zip(tables, counts)])
    video, cls, seg, score = cat('video').long(), cat('cls').long(), cat('seg'), cat('sup')[:, 0]
    N = video.numel()
    # a detection of a video without ground truth (or outside the index) moves to the further class K: no row count changes
    inside = (video >= 0) & (video < nvid) & (cls >= 0) & (cls < K)
    keep = inside & dev['has_gt'][video.clamp(0, max(nvid - 1, 0))]
    cls = torch.where(keep, cls, torch.full_like(cls, K))
    video = torch.where(keep, video, torch.zeros_like(video))
    # stable sorts: descending score keeps equal scores in row order; then the class; then the group (class, video)
    by_score = torch.sort(score, descending=True, stable=True).indices
    by_class = by_score[torch.sort(cls[by_score], stable=True).indices]
    key = cls * nvid + video
    perm = torch.sort(key[by_class], stable=True).indices           # group-sorted position -> position in class order
    by_group = by_class[perm]
    rank_pos = torch.empty(N, dtype=torch.int32, device=device)
    rank_pos[perm] = torch.arange(N, dtype=torch.int32, device=device)
    edges = torch.arange((K + 1) * nvid + 1, device=device)
    pred_start = torch.searchsorted(key[by_group], edges).int()
    class_start = torch.searchsorted(cls[by_class], edges[:K + 1]).int()
    codes, nonfinite = ops.eval_match(seg[by_group].contiguous(), pred_start, dev['gt_seg'], dev['gt_start'],
                                      torch.from_numpy(thr).to(device))
    ap = ops.average_precision(codes, rank_pos, class_start, dev['gt_count']).cpu().numpy()
    if int(nonfinite.item()) != 0:          # final: the read-back above waited for both kernels
        warnings.warn("table_ap: non-finite tIoU (zero-length segments) or a group with too many ground truths; "
                      "evaluating on the CPU instead")
        return ap_reference(_host_columns(tables), gt.columns(), thr, K)
    return ap
