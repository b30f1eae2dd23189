"""CPU: evaluate('WI') -- the Wilderness Impact and the open-set error breakdown -- against the golden results of the
reference's compute_wilderness_impact (tools/pin_wilderness.py -> golden/eval_wi.json), the labelled matching rule of
evaluation/match.py on hand-built cases, otal_eval_match_labeled's argument codes and eval_open's --wi / --stats_json."""
import ctypes
import json
import os
import shutil

import numpy as np
import pytest

from eval_match_cases import TIOUS
from eval_wi_cases import open_detector, stats_counts, stats_outcome, wi_golden, wi_paths

# detections per outcome of the golden fixture with ood_threshold 0.3 at tIoU 0.3 .. 0.7, as the reference's stats count
# them (fp_k2k / fp_k2u include the background detections fp_bg2k / fp_bg2u)
FIXTURE_COUNTS = {"tp_u2u": [7, 3, 2, 2, 1], "tp_k2k": [51, 51, 49, 46, 40], "fp_u2k": [66, 63, 53, 42, 30],
                  "fp_k2k": [508, 511, 523, 537, 555], "fp_k2u": [187, 191, 192, 192, 193],
                  "fp_bg2u": [120, 128, 125, 132, 139], "fp_bg2k": [441, 460, 482, 512, 537]}


@pytest.fixture(scope="module")
def paths(golden_dir):
    return wi_paths(golden_dir)


@pytest.fixture(scope="module")
def golden(paths):
    return wi_golden(paths)


def _equals_golden(det, result, want):
    mWI, avg, wi = result
    assert np.array_equal(stats_outcome(det.stats), np.array(want["outcome"], dtype=np.int8))
    assert stats_counts(det.stats) == want["counts"]
    assert det.stats["num_gt"].dtype == np.float32 and det.stats["num_gt"].tolist() == want["num_gt"]
    assert np.array_equal(det.stats["max_tious"], np.array(want["max_tious"]))
    assert wi.shape == np.array(want["wi"]).shape and np.abs(wi - np.array(want["wi"])).max() < 1e-12
    assert np.abs(mWI - np.array(want["mWI"])).max() < 1e-12 and abs(avg - np.mean(want["mWI"])) < 1e-12
    assert det.wi is wi and det.mWI is mWI and det.average_mWI == avg
    n = len(det.prediction["score"])
    assert sorted(det.stats) == sorted(list(want["counts"]) + ["ood_scores", "scores", "max_tious", "num_gt"])
    assert len(det.stats["ood_scores"]) == len(det.stats["scores"]) == len(det.stats["max_tious"]) == n
    assert det.stats["tp_u2u"].shape == (len(TIOUS), n) and det.stats["fp_bg2k"].shape == (len(TIOUS), 15, n)


@pytest.mark.parametrize("case,thr", [("0.3", 0.3), ("none", None)])
def test_wi_equals_the_reference_on_the_fixture(paths, golden, case, thr):
    det = open_detector(paths, ood_threshold=thr)
    _equals_golden(det, det.evaluate(type="WI"), golden[case])
    if thr == 0.3:
        assert golden[case]["counts"] == FIXTURE_COUNTS
    # detections are numbered video by video in sorted order, file order inside
    order = np.lexsort((np.arange(len(det.prediction["score"])), np.unique(det.prediction["video-id"].astype(str), return_inverse=True)[1].reshape(-1)))
    assert np.array_equal(det.stats["scores"], det.prediction["score"][order])
    assert np.array_equal(det.stats["ood_scores"], det.prediction["ood_score"][order])


def test_set_ood_threshold_gives_the_thresholds_result(paths, golden):
    det = open_detector(paths)
    _equals_golden(det, det.evaluate(type="WI"), golden["none"])
    det.set_ood_threshold(0.3)
    _equals_golden(det, det.evaluate(type="WI"), golden["0.3"])
    det.set_ood_threshold(None)
    _equals_golden(det, det.evaluate(type="WI"), golden["none"])


def test_closed_set_evaluator_asserts(paths):
    from eval_match_cases import detector
    with pytest.raises(AssertionError, match="Wilderness Impact Cannot be Evaluated for Closed Set"):
        detector(paths, "eval_gt_closed.json", openset=False).evaluate(type="WI")


def _run(pred, gt, thresholds=(0.5,), pred_start=None, gt_start=None, n_known=3):
    """pred / gt: rows of (start, end, label), one group unless offsets are given -> (codes, max_tiou, outcome, flags)."""
    from opental_amd.evaluation import match
    pred, gt = np.array(pred, dtype=np.float64).reshape(-1, 3), np.array(gt, dtype=np.float64).reshape(-1, 3)
    pl, gl = pred[:, 2].astype(np.int64), gt[:, 2].astype(np.int64)
    pred_start = [0, len(pred)] if pred_start is None else pred_start
    gt_start = [0, len(gt)] if gt_start is None else gt_start
    codes, top = match.match_labeled_reference(pred[:, :2], pl, pred_start, gt[:, :2], gl, gt_start, list(thresholds))
    assert codes.dtype == np.int32 and top.dtype == np.float64
    flags = match.wi_outcomes(codes, pl, gl, n_known)
    outcome = match.wi_outcome_codes(codes, pl, gl)
    # the seven arrays say what the codes say: one flag per detection, in the class row of the PREDICTION's label
    for idx, key in enumerate(match.WI_OUTCOMES):
        per_class = key in match.WI_PER_CLASS
        assert flags[key].shape == ((len(thresholds), n_known, len(pred)) if per_class else (len(thresholds), len(pred)))
        assert np.array_equal((flags[key].sum(axis=1) if per_class else flags[key]) > 0, outcome == idx), key
        if per_class:
            t, i = np.nonzero(outcome == idx)
            assert (flags[key][t, pl[i] - 1, i] == 1).all() and flags[key].sum() == len(t)
    return codes.tolist(), top, outcome.tolist(), flags


TP_U2U, TP_K2K, FP_U2K, FP_K2K, FP_K2U, FP_BG2U, FP_BG2K, NONE = 0, 1, 2, 3, 4, 5, 6, -1


def test_outcome_names_are_the_references():
    from opental_amd.evaluation.match import WI_OUTCOMES
    assert WI_OUTCOMES == ("tp_u2u", "tp_k2k", "fp_u2k", "fp_k2k", "fp_k2u", "fp_bg2u", "fp_bg2k")


def test_a_wrong_label_does_not_lock():
    codes, top, outcome, flags = _run([(0, 10, 2), (0, 9, 1)], [(0, 10, 1)])
    assert codes == [[0, 0]] and outcome == [[FP_K2K, TP_K2K]]
    assert flags["fp_k2k"][0, 1, 0] == 1 and flags["tp_k2k"][0, 0, 1] == 1      # class row = prediction label - 1
    assert top.tolist() == [1.0, 0.9]


def test_second_true_positive_moves_to_the_next_best_open_ground_truth():
    codes, top, outcome, _ = _run([(0, 10, 1), (0, 10.5, 1)], [(0, 10, 1), (2, 12, 1)])
    assert codes == [[0, 1]] and outcome == [[TP_K2K, TP_K2K]]
    assert top[1] == 10 / 10.5                  # the best tIoU is the locked ground truth's, whatever the match


def test_second_true_positive_without_another_candidate_is_background():
    codes, _, outcome, _ = _run([(0, 10, 1), (0, 10, 1), (0, 10, 0)], [(0, 10, 1), (50, 60, 2)])
    assert codes == [[0, -1, -1]] and outcome == [[TP_K2K, FP_BG2K, FP_BG2U]]


def test_everything_clears_the_threshold_and_is_locked_gives_no_flag():
    codes, _, outcome, flags = _run([(0, 10, 1), (0, 10, 1)], [(0, 10, 1)])
    assert codes == [[0, -2]] and outcome == [[TP_K2K, NONE]]
    assert all(f[..., 1].sum() == 0 for f in flags.values())


def test_unknown_ground_truth_and_unknown_predictions():
    codes, _, outcome, flags = _run([(0, 10, 3), (0, 10, 0), (0, 10, 0), (20, 30, 0), (20, 30, 2)], [(0, 10, 0), (20, 30, 2)])
    # known on unknown (no lock), unknown on unknown (lock), the next finds it locked and the other below the threshold,
    # unknown on known (no lock), known on known
    assert codes == [[0, 0, -1, 1, 1]] and outcome == [[FP_U2K, TP_U2U, FP_BG2U, FP_K2U, TP_K2K]]
    assert flags["fp_u2k"][0, 2, 0] == 1


def test_thresholds_are_independent_problems():
    codes, _, outcome, _ = _run([(0, 10, 1), (0, 12, 1)], [(0, 10, 1), (0, 16, 1)], thresholds=(0.5, 0.8))
    # 0.5: the second takes ground truth 1 (tIoU 0.75); 0.8: ground truth 0 is locked, ground truth 1 is below -> background
    assert codes == [[0, 1], [0, -1]] and outcome == [[TP_K2K, TP_K2K], [TP_K2K, FP_BG2K]]


def test_videos_without_predictions_or_without_ground_truth():
    codes, top, outcome, _ = _run([(0, 10, 1), (0, 10, 2)], [(0, 10, 1), (0, 10, 2)], pred_start=[0, 0, 1, 2, 2],
                                  gt_start=[0, 1, 1, 2, 2])
    # group 0: ground truth and no prediction; 1: a prediction and no ground truth; 2: both; 3: neither
    assert codes == [[-1, 1]] and outcome == [[FP_BG2K, TP_K2K]] and top.tolist() == [0.0, 1.0]


def test_duplicated_ground_truth_segment_goes_to_the_lowest_row():
    gt = [(50, 60, 3), (10, 20, 1), (10, 20, 2)]
    codes, _, outcome, _ = _run([(10, 20, 2), (10, 20, 2), (10, 20, 1), (10, 20, 2), (10, 20, 2)], gt)
    # label 2 on the two equal segments: row 1 first (label 1: a false positive that does not lock) -- and again; label 1 takes
    # and locks row 1; only then does label 2 reach row 2, its own; after that both are locked and row 0 is below
    assert codes == [[1, 1, 1, 2, -1]] and outcome == [[FP_K2K, FP_K2K, TP_K2K, TP_K2K, FP_BG2K]]


def test_labelled_rule_with_equal_labels_is_the_existing_rule():
    from opental_amd.evaluation import match
    from eval_wi_cases import edge_groups
    ps, pl, pstart, gs, gl, gstart = edge_groups("equal")
    codes, _ = match.match_labeled_reference(ps, pl, pstart, gs, gl, gstart, TIOUS)
    assert np.array_equal(codes, match.match_reference(ps, pstart, gs, gstart, TIOUS))
    ps, pl, pstart, gs, gl, gstart = edge_groups("different")
    codes, top = match.match_labeled_reference(ps, pl, pstart, gs, gl, gstart, [0.0])
    # nothing locks and everything clears tIoU 0: every prediction takes its best ground truth
    has_gt = np.repeat(np.diff(gstart) > 0, np.diff(pstart))
    assert (codes[0][has_gt] >= 0).all() and (codes[0][~has_gt] == -1).all()


@pytest.fixture(scope="module")
def lib():
    from opental_amd.csrc import build
    if not os.path.exists(build.LIB):
        build.build(verbose=False)
    from opental_amd._lib import declare
    return declare(ctypes.CDLL(build.LIB))


def test_eval_match_labeled_is_exported_and_abi_is_unchanged(lib):
    assert hasattr(lib, "otal_eval_match_labeled") and lib.otal_abi_version() == 26


def test_eval_match_labeled_argument_errors_do_not_launch(lib):
    one = ctypes.c_void_p(16)       # never dereferenced: argument checks come first
    odd = ctypes.c_void_p(24)       # not 16-byte aligned
    f = lib.otal_eval_match_labeled
    ok = lambda: [one, one, one, one, one, one, one, 1, 5, one, one, one, None]
    for k in (0, 1, 2, 3, 4, 5, 6, 9, 10, 11):                               # every pointer argument in turn
        args = ok()
        args[k] = None
        assert f(*args) == -1, k                                            # OTAL_E_NULL
    for k, value, code in ((7, -1, -2), (8, 0, -2), (8, 33, -7), (0, odd, -7), (3, odd, -7)):
        args = ok()                 # ngroups < 0, nthr < 1: OTAL_E_SHAPE; nthr > 32, unaligned segments: OTAL_E_UNSUPPORTED
        args[k] = value
        assert f(*args) == code, (k, value)
    args = ok()
    args[7] = 0
    assert f(*args) == 0                                                    # no group: success, nothing launched


@pytest.mark.parametrize("module", ["thumos14", "anet"])
def test_eval_open_wi_and_stats_json(paths, golden, tmp_path, capsys, module):
    import importlib
    eval_open = importlib.import_module("opental_amd.%s.eval_open" % module)
    gt_file, classes = paths["eval_gt_open.json"], paths["eval_classes.txt"]
    extra = []
    if module == "anet":            # that driver reads the `validation` subset, one class name per line, tIoU 0.5 .. 0.95
        db = json.load(open(gt_file))
        for v in db["database"].values():
            v["subset"] = "validation"
        gt_file, classes = str(tmp_path / "gt.json"), str(tmp_path / "classes.txt")
        json.dump(db, open(gt_file, "w"))
        open(classes, "w").write("".join(l.split()[1] + "\n" for l in open(paths["eval_classes.txt"]) if l.strip()))
        extra = ["--tious"] + [str(t) for t in TIOUS]
    pred = tmp_path / "split_0" / "detection_results.json"
    pred.parent.mkdir(parents=True)
    shutil.copy(paths["eval_pred.json"], pred)
    pattern = str(tmp_path / "split_{id:d}" / "detection_results.json")
    stats_file = str(tmp_path / "stats.json")
    base = [pattern, gt_file, "--cls_idx_known", classes, "--all_splits", "0", "--open_set", "--ood_scoring", "uncertainty"] + extra
    per_split = eval_open.main(base + ["--wi", "--stats_json", stats_file, "--ood_threshold", "0.3", "--device", "cpu"])
    text = capsys.readouterr().out
    want = golden["0.3"]
    assert np.abs(per_split[0]["wi"] - np.array(want["mWI"])).max() < 1e-12
    for tiou, m in zip(TIOUS, want["mWI"]):
        assert f"WI(tIoU={tiou}): mean={m:.5f}, std=0.00000" in text
    assert f"Average WI = {np.mean(want['mWI']):.5f} (0.00000)" in text
    written = json.load(open(stats_file))
    split = written["splits"]["0"]
    assert split["detections"] == 819 and [r["tiou"] for r in split["thresholds"]] == TIOUS
    det = open_detector(paths, ood_threshold=0.3)
    det.evaluate(type="WI")
    ood = det.stats["ood_scores"]               # in the order of the outcome codes
    for tidx, row in enumerate(split["thresholds"]):
        assert {k: v for k, v in row["counts"].items() if k != "none"} == {k: v[tidx] for k, v in FIXTURE_COUNTS.items()}
        assert row["counts"]["none"] == 0
        assert row["ood_mean"]["none"] is None and row["ood_ci"]["none"] is None
        assert 0 < row["ood_mean"]["tp_u2u"] < 0.3 <= row["ood_mean"]["tp_k2k"] and row["ood_ci"]["fp_k2k"] > 0
    # mean and half-width of one outcome, from the golden codes
    mask = np.array(want["outcome"][0]) == 1
    assert abs(split["thresholds"][0]["ood_mean"]["tp_k2k"] - ood[mask].mean()) < 1e-12
    assert abs(split["thresholds"][0]["ood_ci"]["tp_k2k"] - ood[mask].std() / np.sqrt(mask.sum()) * 1.96) < 1e-12
    # without --wi the summary and the text file are the driver's as before; --wi needs the open-set protocol
    eval_open.main(base)
    assert "WI(" not in capsys.readouterr().out
    with pytest.raises(SystemExit):
        eval_open.main([pattern, gt_file, "--cls_idx_known", classes, "--all_splits", "0", "--wi"])
