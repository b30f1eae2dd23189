"""Shared inputs of test_eval_wi_cpu.py / test_eval_wi_gpu.py: the golden fixture of evaluate('WI'), the outcome codes of a
stats dict, and seeded labelled groups at the chunk edges of the 64-lane kernel."""
import json
import os

import numpy as np

from eval_match_cases import TIOUS, detector, fixture_paths

GT_COUNTS = (1, 63, 64, 65, 130)            # ground truths per group: the chunk edges of a 64-lane mapping
PRED_COUNTS = (1, 64, 65, 200)              # predictions per group: the edges of the batch of 64
LABEL_REGIMES = ("equal", "different", "mixed")


def wi_paths(golden_dir):
    paths = fixture_paths(golden_dir)
    paths["eval_wi.json"] = os.path.join(golden_dir, "eval_wi.json")
    return paths


def wi_golden(paths):
    return json.load(open(paths["eval_wi.json"]))


def open_detector(paths, **kw):
    return detector(paths, "eval_gt_open.json", openset=True, ood_scoring="uncertainty", **kw)


def stats_outcome(stats):
    """ANETdetection.stats -> int8 (nthr, N): the index into match.WI_OUTCOMES of each detection's flag, -1 for none.  The
    stats carry the background flags twice (fp_bg2u also in fp_k2u, fp_bg2k also in fp_k2k, as the reference returns them);
    the background flags come last in WI_OUTCOMES and win."""
    from opental_amd.evaluation.match import WI_OUTCOMES
    per_det = {k: (stats[k].sum(axis=1) if stats[k].ndim == 3 else stats[k]) for k in WI_OUTCOMES}
    outcome = np.full(per_det["tp_u2u"].shape, -1, dtype=np.int8)
    for idx, key in enumerate(WI_OUTCOMES):
        assert set(np.unique(per_det[key]).tolist()) <= {0.0, 1.0}, key
        outcome[per_det[key] > 0] = idx
    return outcome


def stats_counts(stats):
    from opental_amd.evaluation.match import WI_OUTCOMES
    return {k: stats[k].reshape(stats[k].shape[0], -1).sum(axis=1).astype(int).tolist() for k in WI_OUTCOMES}


def labels_for(regime, rs, npred, ngt):
    if regime == "equal":
        return np.ones(npred, np.int32), np.ones(ngt, np.int32)
    if regime == "different":
        return np.ones(npred, np.int32), np.full(ngt, 2, np.int32)
    return rs.randint(0, 4, npred).astype(np.int32), rs.randint(0, 4, ngt).astype(np.int32)


def edge_groups(regime, seed=11):
    """Two groups per (ground-truth count, prediction count), one group with predictions and no ground truth and one with
    ground truth and no predictions: 42 groups at continuous random times (no two tIoU tie); 70 % of the predictions are
    jittered copies of a ground truth, so that repeats on one ground truth are common.
    -> (pred_seg, pred_label, pred_start, gt_seg, gt_label, gt_start)."""
    rs = np.random.RandomState(seed)
    shapes = [(g, p) for g in GT_COUNTS for p in PRED_COUNTS] * 2
    shapes.insert(7, (0, 70))
    shapes.insert(23, (70, 0))
    pred, gt, plab, glab, pstart, gstart = [], [], [], [], [0], [0]
    for ngt, npred in shapes:
        start = rs.uniform(0, 60, ngt)
        length = rs.uniform(1, 20, ngt)
        gt.append(np.stack([start, start + length], 1))
        if ngt:
            j = rs.randint(0, ngt, npred)
            s = np.where(rs.rand(npred) < 0.7, start[j] + rs.normal(0, 0.2, npred) * length[j], rs.uniform(0, 60, npred))
            pred.append(np.stack([s, s + length[j] * rs.uniform(0.7, 1.4, npred)], 1))
        else:
            s = rs.uniform(0, 60, npred)
            pred.append(np.stack([s, s + rs.uniform(1, 20, npred)], 1))
        pl, gl = labels_for(regime, rs, npred, ngt)
        plab.append(pl); glab.append(gl)
        pstart.append(pstart[-1] + npred); gstart.append(gstart[-1] + ngt)
    return (np.concatenate(pred), np.concatenate(plab), np.array(pstart, np.int32),
            np.concatenate(gt), np.concatenate(glab), np.array(gstart, np.int32))
