"""tools/pin_wilderness.py -- pins evaluate('WI') (Wilderness Impact and the open-set error breakdown) against the reference's
compute_wilderness_impact (AFSD/evaluation/eval_detection.py:604-728); runs on the CPU where the reference source tree is
available, never on the GPU machine.  Nothing of the reference is written into the repository; the golden file holds the
numbers its function returned on the committed tests/golden/eval_*.json fixture.

The reference's wrapper visits the videos in list(set(...)) order, which changes from process to process and moves the WI value;
here its function is called with video_list = sorted(set(...)), the order opental_amd defines.  `np.float` (removed in numpy
1.24) is restored in THIS process only, as oracle/pin_evaluation.py does.

For ood_threshold 0.3 and None (scoring 'uncertainty', tIoU 0.3 .. 0.7) it asserts that the fixture has no two ground truths
of a video with equal tIoU at or above the lowest threshold (where the reference's choice would belong to the numpy build),
that our flags, max_tious and num_gt equal the reference's exactly and wi to < 1e-12, and writes tests/golden/eval_wi.json:

    "tious", and per case ("0.3", "none"):
      "wi" (nthr, K), "mWI" (nthr,)
      "outcome" (nthr, N) one code per threshold and detection: the index into match.WI_OUTCOMES, -1 for none
      "counts"  per stats key, (nthr,) the number of flagged detections AS THE REFERENCE RETURNS THEM: its stats hold the
                arrays that :712-713 fold in place, so fp_k2u / fp_k2k include the background detections
      "max_tious" (N,), "num_gt" (K + 1,)

and appends a line to tests/golden/PIN_REPORT_wilderness.txt.

    python -m tools.pin_wilderness
"""
import json
import os
import sys

sys.dont_write_bytecode = True
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
GOLD = os.path.join(REPO, "tests", "golden")

import numpy as np

TIOUS = [0.3, 0.4, 0.5, 0.6, 0.7]
CASES = (("0.3", 0.3), ("none", None))


def assert_no_ties(det, lowest):
    """No video has two ground truths with the same tIoU >= `lowest` against one of its detections."""
    from opental_amd.evaluation import match
    from opental_amd.evaluation.utils_eval import segment_iou
    plan = match.plan_split(det.prediction, det.ground_truth)
    pred_seg, pred_start, gt_seg, gt_start = plan.arrays()
    for g in range(plan.ngroups):
        for i in range(pred_start[g], pred_start[g + 1]):
            tiou = segment_iou(pred_seg[i], gt_seg[gt_start[g]:gt_start[g + 1]])
            top = tiou[~(tiou < lowest)]
            assert len(np.unique(top)) == len(top), ("tie", g, i, top)


def main():
    from oracle.pin_evaluation import REF
    from opental_amd.evaluation import match
    from opental_amd.evaluation.eval_detection import ANETdetection as OurDet
    np.float = float                      # see the module docstring
    sys.path.insert(0, REF)
    import copy
    from AFSD.evaluation import eval_detection as ref_mod
    ref_mod.tqdm = lambda it, **kw: it    # no progress bar in the report

    paths = {k: os.path.join(GOLD, k) for k in ("eval_classes.txt", "eval_gt_open.json", "eval_pred.json")}
    common = dict(ground_truth_filename=paths["eval_gt_open.json"], prediction_filename=paths["eval_pred.json"],
                  cls_idx_detection=paths["eval_classes.txt"], subset=["test"], tiou_thresholds=TIOUS, dataset="thumos14",
                  openset=True, ood_scoring="uncertainty")
    golden, report = {"tious": TIOUS}, []
    for name, thr in CASES:
        ref = ref_mod.ANETdetection(ood_threshold=thr, **common)
        our = OurDet(ood_threshold=thr, **common)
        assert_no_ties(our, min(TIOUS))
        known = copy.deepcopy(ref.activity_index)
        del known['__unknown__']
        r_wi, r_stats = ref_mod.compute_wilderness_impact(ref.ground_truth, ref.prediction, sorted(set(ref.video_lst)), known,
                                                          tiou_thresholds=TIOUS)
        o_mwi, o_avg, o_wi = our.evaluate(type="WI")
        o_stats = our.stats
        for key in match.WI_OUTCOMES:
            assert r_stats[key].shape == o_stats[key].shape and np.array_equal(r_stats[key], o_stats[key]), key
        for key in ("ood_scores", "scores", "max_tious", "num_gt"):
            assert np.array_equal(np.asarray(r_stats[key], dtype=np.float64), np.asarray(o_stats[key], dtype=np.float64)), key
        assert r_stats["num_gt"].dtype == o_stats["num_gt"].dtype == np.float32
        d = float(np.abs(r_wi - o_wi).max())
        assert d < 1e-12, d
        # one code per (threshold, detection) from the REFERENCE's arrays: the unfolded flag where two are set
        per_det = {k: (r_stats[k].sum(axis=1) if r_stats[k].ndim == 3 else r_stats[k]) for k in match.WI_OUTCOMES}
        outcome = np.full(per_det["tp_u2u"].shape, -1, dtype=np.int8)
        for idx, key in enumerate(match.WI_OUTCOMES):           # the background flags come last and overwrite their folds
            assert set(np.unique(per_det[key]).tolist()) <= {0.0, 1.0}, key
            outcome[per_det[key] > 0] = idx
        lp = our.prediction['label'][our._plan('split').order]
        for idx, key in enumerate(match.WI_OUTCOMES):           # the codes lose nothing: they give the reference's arrays back
            want = (outcome == idx) | ((outcome == {"fp_k2u": 5, "fp_k2k": 6}.get(key, -9)))
            assert np.array_equal(per_det[key] > 0, want), key
            if r_stats[key].ndim == 3:
                t, i = np.nonzero(per_det[key] > 0)
                assert (r_stats[key][t, lp[i] - 1, i] == 1).all(), key
        counts = {k: per_det[k].sum(axis=-1).astype(int).tolist() for k in match.WI_OUTCOMES}
        golden[name] = {"wi": r_wi.tolist(), "mWI": r_wi.mean(axis=1).tolist(), "outcome": outcome.tolist(), "counts": counts,
                        "max_tious": [float(x) for x in r_stats["max_tious"]], "num_gt": r_stats["num_gt"].tolist()}
        report.append(f"wilderness impact, ood_threshold {name}: {outcome.shape[1]} detections, none-outcomes "
                      f"{int((outcome < 0).sum())}, max|ref-ours| wi = {d:.1e}; mWI {[round(float(x), 4) for x in r_wi.mean(axis=1)]}; "
                      f"counts at tIoU {TIOUS[0]}: " + ", ".join(f"{k} {v[0]}" for k, v in counts.items()))
    with open(os.path.join(GOLD, "eval_wi.json"), "w") as f:
        json.dump(golden, f, separators=(",", ":"))
    with open(os.path.join(GOLD, "PIN_REPORT_wilderness.txt"), "a") as f:
        f.write("\n".join(report) + "\n")
    print("\n".join(report))


if __name__ == "__main__":
    main()
