"""Shared inputs of test_eval_match_cpu.py / test_eval_match_gpu.py: seeded synthetic result sets in the evaluator's column
layout (parallel arrays, as ANETdetection imports them) and the golden fixture's paths."""
import os

import numpy as np

TIOUS = [0.3, 0.4, 0.5, 0.6, 0.7]
NCLASS = 15


def fixture_paths(golden_dir):
    return {k: os.path.join(golden_dir, k) for k in ("eval_classes.txt", "eval_gt_open.json", "eval_gt_closed.json",
                                                      "eval_pred.json", "eval_expected.json")}


def detector(paths, gt, **kw):
    from opental_amd.evaluation.eval_detection import ANETdetection
    return ANETdetection(ground_truth_filename=paths[gt], prediction_filename=paths["eval_pred.json"],
                         cls_idx_detection=paths["eval_classes.txt"], subset=["test"], tiou_thresholds=TIOUS,
                         dataset="thumos14", **kw)


def _tables(gt_rows, pred_rows):
    """rows of (video, start, end, label[, score, ood]) -> the evaluator's two column tables."""
    gt = {'video-id': np.array([r[0] for r in gt_rows], dtype=object),
          't-start': np.array([r[1] for r in gt_rows], dtype=np.float64),
          't-end': np.array([r[2] for r in gt_rows], dtype=np.float64),
          'label': np.array([r[3] for r in gt_rows], dtype=np.int64)}
    pred = {'video-id': np.array([r[0] for r in pred_rows], dtype=object),
            't-start': np.array([r[1] for r in pred_rows], dtype=np.float64),
            't-end': np.array([r[2] for r in pred_rows], dtype=np.float64),
            'label': np.array([r[3] for r in pred_rows], dtype=np.int64),
            'score': np.array([r[4] for r in pred_rows], dtype=np.float64),
            'ood_score': np.array([r[5] for r in pred_rows], dtype=np.float64)}
    return gt, pred


def continuous_set(seed=0, nvideos=12, gt_counts=None, pred_counts=None):
    """Videos with 1 .. 150 ground truths and 0 .. 300 detections at continuous random times (no two tIoU tie); about half
    of the detections are jittered copies of a ground truth, so that matches, repeats and misses all occur.  Labels 0 ..
    NCLASS (0 = '__unknown__'), every class has ground truth.  Detections of the videos interleave in file order."""
    rs = np.random.RandomState(seed)
    gt_rows, pred_rows = [], []
    for v in range(nvideos):
        name = "video_%03d" % ((v * 7) % nvideos)            # file order differs from sorted order
        ngt = int(rs.randint(1, 151)) if gt_counts is None else gt_counts[v]
        npred = int(rs.randint(0, 301)) if pred_counts is None else pred_counts[v]
        start = rs.uniform(0, 300, ngt)
        length = rs.uniform(1, 20, ngt)
        for j in range(ngt):
            label = (len(gt_rows) % (NCLASS + 1))
            gt_rows.append((name, start[j], start[j] + length[j], label))
        for _ in range(npred):
            if ngt and rs.rand() < 0.5:
                j = rs.randint(ngt)
                s = start[j] + rs.normal(0, 0.25) * length[j]
                e = s + length[j] * rs.uniform(0.6, 1.5)
            else:
                s = rs.uniform(0, 300)
                e = s + rs.uniform(1, 20)
            pred_rows.append((name, s, e, int(rs.randint(0, NCLASS + 1)), rs.rand(), rs.rand()))
    order = rs.permutation(len(pred_rows))
    return _tables(gt_rows, [pred_rows[i] for i in order])


def grid_set(seed=2, nvideos=30, max_gt=40, max_pred=200, span=12):
    """Segments on a small integer grid: equal tIoU between candidates (ties), tIoU exactly on a threshold and ground truths
    that all clear a threshold (-2) are common.  Compare with match_reference only: the CPU loops are undefined under ties."""
    rs = np.random.RandomState(seed)
    gt_rows, pred_rows = [], []
    for v in range(nvideos):
        name = "grid_%02d" % v
        for _ in range(int(rs.randint(1, max_gt + 1))):
            s = int(rs.randint(0, span))
            gt_rows.append((name, float(s), float(s + rs.randint(1, 11)), int(rs.randint(0, 4))))
        for _ in range(int(rs.randint(0, max_pred + 1))):
            s = int(rs.randint(0, span))
            pred_rows.append((name, float(s), float(s + rs.randint(1, 11)), int(rs.randint(0, 4)),
                              float(rs.randint(0, 20)) / 20.0, rs.rand()))
    return _tables(gt_rows, pred_rows)


def count_grid_events(plan, thresholds):
    """(ties, exact hits, -2 results) of a plan under match_reference's rule: a tie is a prediction whose two best untaken
    candidates have equal tIoU; an exact hit is a candidate with tIoU == thr."""
    from opental_amd.evaluation.match import match_reference
    from opental_amd.evaluation.utils_eval import segment_iou
    pred_seg, pred_start, gt_seg, gt_start = plan.arrays()
    codes = match_reference(pred_seg, pred_start, gt_seg, gt_start, thresholds)
    ties = exact = 0
    for g in range(plan.ngroups):
        g0, g1 = gt_start[g], gt_start[g + 1]
        if g1 == g0:
            continue
        for t, thr in enumerate(thresholds):
            taken = np.zeros(g1 - g0, dtype=bool)
            for i in range(pred_start[g], pred_start[g + 1]):
                tiou = segment_iou(pred_seg[i], gt_seg[g0:g1])
                cand = ~(tiou < thr) & ~taken
                if cand.any():
                    vals = np.sort(tiou[cand])
                    ties += len(vals) > 1 and vals[-1] == vals[-2]
                    exact += bool((tiou[cand] == thr).any())
                if codes[t, i] >= 0:
                    taken[codes[t, i] - g0] = True
    return int(ties), int(exact), int((codes == -2).sum())
