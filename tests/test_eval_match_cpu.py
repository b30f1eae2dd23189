"""CPU: the matching rule of opental_amd/evaluation/match.py (match_reference + the two planners) against the evaluator's
own loops (split_results_by_gt, compute_average_precision_detection), its tie and exact-threshold behaviour,
ANETdetection.set_ood_threshold, the threshold search, eval_open's --device flag and otal_eval_match's argument codes."""
import ctypes
import json
import os

import numpy as np
import pytest

from eval_match_cases import NCLASS, TIOUS, continuous_set, detector, fixture_paths


@pytest.fixture(scope="module")
def paths(golden_dir):
    return fixture_paths(golden_dir)


def _check_against_loops(pred, gt, classes):
    """-> the number of -2 results of the split pass."""
    from opental_amd.evaluation import match
    from opental_amd.evaluation.eval_detection import compute_average_precision_detection, split_results_by_gt
    from opental_amd.evaluation.utils_eval import interpolated_prec_rec
    plan = match.plan_split(pred, gt)
    codes = match.match_reference(*plan.arrays(), TIOUS)
    got = match.split_lists(plan, codes, pred, gt, len(TIOUS))
    want = split_results_by_gt(pred, gt, sorted(set(gt['video-id'].tolist())), TIOUS)
    for g3, w3 in zip(got, want):
        for t in range(len(TIOUS)):
            for key in ('bg', 'known', 'unknown'):
                assert len(g3[t][key]) == len(w3[t][key]), (t, key)
                assert all(a == b for a, b in zip(g3[t][key], w3[t][key])), (t, key)
    aplan = match.plan_ap(pred, gt, classes)
    ap = match.average_precision(aplan, aplan.unsort(match.match_reference(*aplan.arrays(), TIOUS)), classes, len(TIOUS),
                                 interpolated_prec_rec)
    for c in classes:
        rows = lambda table: {k: v[table['label'] == c] for k, v in table.items()}
        want_ap = compute_average_precision_detection(rows(gt), rows(pred), TIOUS)
        assert (ap[:, c - 1] == want_ap).all(), (c, ap[:, c - 1], want_ap)
    return int((codes == -2).sum())


@pytest.mark.parametrize("gt_file,openset,minus2", [("eval_gt_open.json", True, None), ("eval_gt_closed.json", False, 26)])
def test_rule_equals_the_loops_on_the_fixture(paths, gt_file, openset, minus2):
    det = detector(paths, gt_file, openset=openset)
    n = _check_against_loops(det.prediction, det.ground_truth, list(det.activity_index.values()))
    if minus2 is not None:
        assert n == minus2          # predictions whose ground truths all clear the threshold and are all taken


def test_rule_equals_the_loops_on_continuous_segments():
    gt, pred = continuous_set(seed=0)
    assert len(set(gt['video-id'].tolist())) == 12 and len(pred['score']) > 1000
    _check_against_loops(pred, gt, list(range(NCLASS + 1)))


def test_equal_tiou_takes_the_first_ground_truth_in_file_order():
    """Two identical ground truths of different labels (THUMOS14 annotates CliffDiving and Diving with one segment): the first
    prediction takes the first row, the next prediction the second, the third finds both taken."""
    from opental_amd.evaluation.match import match_reference
    gt_seg = np.array([[50.0, 60.0], [10.0, 20.0], [10.0, 20.0]])
    pred_seg = np.array([[10.0, 20.0], [11.0, 20.0], [10.0, 19.0]])
    codes = match_reference(pred_seg, [0, 3], gt_seg, [0, 3], [0.5])
    assert codes.dtype == np.int32 and codes.tolist() == [[1, 2, -1]]
    # without the far ground truth every ground truth clears the threshold: the third prediction is the -2 case
    assert match_reference(pred_seg, [0, 3], gt_seg[1:], [0, 2], [0.5]).tolist() == [[0, 1, -2]]


def test_tiou_equal_to_the_threshold_matches():
    from opental_amd.evaluation.match import match_reference
    codes = match_reference(np.array([[0.0, 10.0]]), [0, 1], np.array([[0.0, 5.0]]), [0, 1], [0.5, 0.5 + 1e-12])
    assert codes.tolist() == [[0], [-1]]        # the test is `not (tiou < thr)`


def test_groups_without_ground_truth_or_predictions():
    from opental_amd.evaluation.match import match_reference
    codes = match_reference(np.array([[0.0, 1.0], [0.0, 1.0]]), [0, 1, 1, 2], np.array([[0.0, 1.0]]), [0, 0, 1, 1], [0.3])
    assert codes.tolist() == [[-1, -1]]


def test_set_ood_threshold_equals_a_fresh_evaluator(paths):
    want = json.load(open(paths["eval_expected.json"]))
    det = detector(paths, "eval_gt_open.json", openset=True, ood_scoring="uncertainty")
    closed = det.evaluate(type="AP")
    det.set_ood_threshold(0.3)
    mAP, avg, ap = det.evaluate(type="AP")
    fresh = detector(paths, "eval_gt_open.json", openset=True, ood_scoring="uncertainty", ood_threshold=0.3).evaluate(type="AP")
    assert np.array_equal(mAP, fresh[0]) and avg == fresh[1] and np.array_equal(ap, fresh[2])
    assert np.abs(mAP - np.array(want["open_ap_threshold_0.3"]["mAP"])).max() < 1e-12
    assert np.abs(ap[:, -1] - np.array(want["open_ap_threshold_0.3"]["ap_unknown_column"])).max() < 1e-12
    assert not np.array_equal(mAP, closed[0])
    det.set_ood_threshold(None)
    again = det.evaluate(type="AP")
    assert np.array_equal(again[0], closed[0]) and again[1] == closed[1] and np.array_equal(again[2], closed[2])


def test_search_equals_one_evaluator_per_candidate(paths):
    from opental_amd.thumos14.search_param import candidates, search
    cand = np.concatenate([[0.1, 0.3, 0.5], candidates()])      # the fixture's scores spread below the driver's 0.8 .. 0.98
    assert len(candidates()) == 10 and abs(candidates()[0] - 0.8) < 1e-12 and abs(candidates()[-1] - 0.98) < 1e-12
    det = detector(paths, "eval_gt_open.json", openset=True, ood_scoring="uncertainty", device="cpu")
    best, best_mAP, all_mAPs = search(det, cand)
    brute = [detector(paths, "eval_gt_open.json", openset=True, ood_scoring="uncertainty", ood_threshold=c).evaluate(type="AP")[1]
             for c in cand]
    assert all_mAPs == brute and len(set(brute)) > 1
    assert best == cand[int(np.argmax(brute))] and best_mAP == max(brute)


def test_eval_open_device_cpu_writes_the_same_files(paths, tmp_path):
    import shutil
    from opental_amd.thumos14 import eval_open
    texts = []
    for extra in ([], ["--device", "cpu"]):
        pred = tmp_path / ("d%d" % len(extra)) / "split_0" / "detection_results.json"
        pred.parent.mkdir(parents=True)
        shutil.copy(paths["eval_pred.json"], pred)
        pattern = str(pred.parent.parent / "split_{id:d}" / "detection_results.json")
        eval_open.main([pattern, paths["eval_gt_open.json"], "--cls_idx_known", paths["eval_classes.txt"], "--all_splits", "0",
                        "--open_set", "--ood_scoring", "uncertainty"] + extra)
        eval_open.main([pattern, paths["eval_gt_closed.json"], "--cls_idx_known", paths["eval_classes.txt"], "--all_splits", "0"]
                       + extra)
        texts.append((open(pred.parent / "eval_open.txt").read(), open(pred.parent / "eval.txt").read()))
    assert texts[0] == texts[1] and texts[0][0].count("\n") == 6


def test_unknown_device_is_refused(paths):
    with pytest.raises(ValueError):
        detector(paths, "eval_gt_open.json", openset=True, device="tpu")


def test_eval_match_argument_errors_do_not_launch():
    from opental_amd.csrc import build
    if not os.path.exists(build.LIB):
        build.build(verbose=False)
    from opental_amd._lib import declare
    lib = declare(ctypes.CDLL(build.LIB))
    one = ctypes.c_void_p(16)       # never dereferenced: argument checks come first
    odd = ctypes.c_void_p(24)       # not 16-byte aligned
    f = lib.otal_eval_match
    for k in (0, 1, 2, 3, 4, 7, 8):                                          # every pointer argument in turn
        args = [one, one, one, one, one, 1, 5, one, one, None]
        args[k] = None
        assert f(*args) == -1, k                                            # OTAL_E_NULL
    assert f(one, one, one, one, one, -1, 5, one, one, None) == -2          # OTAL_E_SHAPE: ngroups < 0
    assert f(one, one, one, one, one, 1, 0, one, one, None) == -2           # OTAL_E_SHAPE: nthr < 1
    assert f(one, one, one, one, one, 1, 33, one, one, None) == -7          # OTAL_E_UNSUPPORTED: nthr > 32
    assert f(odd, one, one, one, one, 1, 5, one, one, None) == -7           # OTAL_E_UNSUPPORTED: unaligned segments
    assert f(one, one, one, one, one, 0, 5, one, one, None) == 0            # no group: success, nothing launched
