"""GPU: otal_eval_match (csrc/eval.hip) against match_reference, code for code (int32, exact), and ANETdetection(device='cuda')
against the golden results of the reference evaluator."""
import json
import warnings

import numpy as np
import pytest

from eval_match_cases import TIOUS, count_grid_events, detector, fixture_paths, grid_set

pytestmark = pytest.mark.gpu

SCORINGS = ["uncertainty", "confidence", "uncertainty_actionness", "a_by_inv_u", "u_by_inv_a", "half_au"]


@pytest.fixture(scope="module")
def paths(golden_dir):
    return fixture_paths(golden_dir)


def _device_equals_reference(arrays, thresholds):
    from opental_amd.evaluation.match import match_device, match_reference
    want = match_reference(*arrays, thresholds)
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message="eval_match")      # a fall-back to the CPU warns: the codes must be the kernel's
        got = match_device(*arrays, thresholds)
    assert got.dtype == np.int32 and got.shape == want.shape
    assert np.array_equal(got, want), np.argwhere(got != want)[:10]
    return want


@pytest.mark.parametrize("gt_file,openset", [("eval_gt_open.json", True), ("eval_gt_closed.json", False)])
def test_fixture_under_both_groupings(paths, gt_file, openset):
    from opental_amd.evaluation import match
    det = detector(paths, gt_file, openset=openset)
    codes = _device_equals_reference(match.plan_split(det.prediction, det.ground_truth).arrays(), TIOUS)
    assert (codes >= 0).any() and (codes == -1).any()
    if not openset:
        assert int((codes == -2).sum()) == 26
    codes = _device_equals_reference(match.plan_ap(det.prediction, det.ground_truth, det.activity_index.values()).arrays(), TIOUS)
    assert (codes >= 0).any() and (codes == -1).any()


GT_COUNTS = (0, 1, 2, 63, 64, 65, 128, 129, 150)     # the chunk edges of a 64-lane mapping
PRED_COUNTS = (0, 1, 300)


@pytest.fixture(scope="module")
def edge_groups():
    """One group per (ground-truth count, prediction count), continuous times."""
    rs = np.random.RandomState(7)
    pred, gt, pstart, gstart = [], [], [0], [0]
    for ngt in GT_COUNTS:
        for npred in PRED_COUNTS:
            start = rs.uniform(0, 60, ngt)
            length = rs.uniform(1, 20, ngt)
            g = np.stack([start, start + length], 1)
            if ngt:
                j = rs.randint(0, ngt, npred)
                s = np.where(rs.rand(npred) < 0.7, start[j] + rs.normal(0, 0.2, npred) * length[j], rs.uniform(0, 60, npred))
                p = np.stack([s, s + length[j] * rs.uniform(0.7, 1.4, npred)], 1)
            else:
                s = rs.uniform(0, 60, npred)
                p = np.stack([s, s + rs.uniform(1, 20, npred)], 1)
            pred.append(p); gt.append(g)
            pstart.append(pstart[-1] + npred); gstart.append(gstart[-1] + ngt)
    return (np.concatenate(pred), np.array(pstart, np.int32), np.concatenate(gt), np.array(gstart, np.int32))


@pytest.mark.parametrize("nthr", [1, 5, 10, 32])
def test_chunk_edges_and_threshold_counts(edge_groups, nthr):
    thresholds = [0.5] if nthr == 1 else np.linspace(0.05, 0.95, nthr)
    codes = _device_equals_reference(edge_groups, thresholds)
    assert (codes >= 0).sum() > 100 and (codes == -1).any()


def test_integer_grid_with_ties_exact_hits_and_all_taken():
    from opental_amd.evaluation import match
    gt, pred = grid_set(seed=2)
    plan = match.plan_split(pred, gt)
    thresholds = [0.25, 0.5, 0.75]          # tIoU of integer segments: ratios of small integers, these three occur exactly
    ties, exact, minus2 = count_grid_events(plan, thresholds)
    print("integer grid: %d ties, %d exact-threshold hits, %d results of -2" % (ties, exact, minus2))
    assert ties > 0 and exact > 0 and minus2 > 0
    codes = _device_equals_reference(plan.arrays(), thresholds)
    assert int((codes == -2).sum()) == minus2
    _device_equals_reference(match.plan_ap(pred, gt, range(4)).arrays(), thresholds)


def test_many_small_groups():
    rs = np.random.RandomState(3)
    n = 2000
    start = rs.uniform(0, 100, n)
    gt = np.stack([start, start + rs.uniform(2, 10, n)], 1)
    j = np.repeat(np.arange(n), 3)
    s = gt[j, 0] + rs.normal(0, 1.0, 3 * n)
    pred = np.stack([s, s + (gt[j, 1] - gt[j, 0]) * rs.uniform(0.7, 1.3, 3 * n)], 1)
    codes = _device_equals_reference((pred, np.arange(n + 1, dtype=np.int32) * 3, gt, np.arange(n + 1, dtype=np.int32)), TIOUS)
    assert (codes[:, -3:] >= 0).any() and len(np.unique(codes[codes >= 0])) > n // 2


def test_group_at_and_above_the_ground_truth_limit():
    """1024 ground truths of one group are the most one wave keeps; one more counts into the counter (all its predictions -1)
    and match_device answers from match_reference."""
    import torch
    from opental_amd.common import ops
    from opental_amd.evaluation.match import match_device, match_reference
    rs = np.random.RandomState(5)
    for ngt in (1024, 1025):
        start = np.sort(rs.uniform(0, 5000, ngt))
        gt = np.stack([start, start + rs.uniform(1, 4, ngt)], 1)
        pred = gt[[0, ngt - 1, ngt - 1, ngt // 2]] + 0.01
        arrays = (pred, np.array([0, 4], np.int32), gt, np.array([0, ngt], np.int32))
        want = match_reference(*arrays, TIOUS)
        assert want[0][[0, 1, 3]].tolist() == [0, ngt - 1, ngt // 2] and want[0][2] != ngt - 1
        if ngt == 1024:
            _device_equals_reference(arrays, TIOUS)
            continue
        dev = [torch.from_numpy(a).cuda() for a in arrays]
        out, counter = ops.eval_match(*dev, torch.tensor(TIOUS, dtype=torch.float64, device="cuda"))
        assert int(counter.item()) == 1 and bool((out == -1).all())
        with pytest.warns(UserWarning, match="eval_match"):
            assert np.array_equal(match_device(*arrays, TIOUS), want)


def test_evaluator_on_the_device_reproduces_the_reference(paths):
    want = json.load(open(paths["eval_expected.json"]))
    mAP, avg, ap = detector(paths, "eval_gt_closed.json", openset=False, device="cuda").evaluate(type="AP")
    assert np.abs(ap - np.array(want["closed"]["ap"])).max() < 1e-12
    assert np.abs(mAP - np.array(want["closed"]["mAP"])).max() < 1e-12 and abs(avg - want["closed"]["average_mAP"]) < 1e-12
    for scoring in SCORINGS:
        det = detector(paths, "eval_gt_open.json", openset=True, ood_scoring=scoring, device="cuda")
        det.pre_evaluate()
        roc, pr, far = det.evaluate(type="AUC")
        osdr = det.evaluate(type="OSDR")
        w = want["open"][scoring]
        n_fg = [len(det.eval_data[0][t]["known"]) + len(det.eval_data[0][t]["unknown"]) for t in range(len(TIOUS))]
        assert n_fg == w["matched_foreground"]
        for got, key in ((roc, "auc_roc"), (pr, "auc_pr"), (far, "far_95"), (osdr, "osdr")):
            assert got.dtype == np.float32
            assert np.abs(got - np.array(w[key], np.float32)).max() < 1e-6, (scoring, key)
    det = detector(paths, "eval_gt_open.json", openset=True, ood_scoring="uncertainty", ood_threshold=0.3, device="cuda")
    mAP, _, ap = det.evaluate(type="AP")
    assert np.abs(mAP - np.array(want["open_ap_threshold_0.3"]["mAP"])).max() < 1e-12
    assert np.abs(ap[:, -1] - np.array(want["open_ap_threshold_0.3"]["ap_unknown_column"])).max() < 1e-12


def test_search_on_the_device_equals_the_cpu_search(paths):
    from opental_amd.thumos14.search_param import candidates, search
    cand = np.concatenate([[0.1, 0.3, 0.5], candidates()])
    res = [search(detector(paths, "eval_gt_open.json", openset=True, ood_scoring="uncertainty", device=d), cand)
           for d in ("cuda", "cpu")]
    assert res[0][0] == res[1][0] and res[0][1] == res[1][1] and res[0][2] == res[1][2]
    assert len(set(res[0][2])) > 1


def test_eval_open_device_cuda_writes_the_same_files(paths, tmp_path):
    import shutil
    from opental_amd.thumos14 import eval_open
    texts = []
    for extra in ([], ["--device", "cuda"]):
        pred = tmp_path / ("d%d" % len(extra)) / "split_0" / "detection_results.json"
        pred.parent.mkdir(parents=True)
        shutil.copy(paths["eval_pred.json"], pred)
        pattern = str(pred.parent.parent / "split_{id:d}" / "detection_results.json")
        eval_open.main([pattern, paths["eval_gt_open.json"], "--cls_idx_known", paths["eval_classes.txt"], "--all_splits", "0",
                        "--open_set", "--ood_scoring", "uncertainty"] + extra)
        texts.append(open(pred.parent / "eval_open.txt").read())
    assert texts[0] == texts[1]


def test_non_finite_tiou_counts_and_falls_back(paths, tmp_path):
    """A zero-length prediction on a zero-length ground truth at the same instant: tIoU = 0 / 0."""
    import torch
    from opental_amd.common import ops
    names = [l.split()[1] for l in open(paths["eval_classes.txt"]).read().splitlines() if l.strip()]
    pred_seg = torch.tensor([[5.0, 5.0], [10.0, 19.0]], dtype=torch.float64, device="cuda")
    gt_seg = torch.tensor([[5.0, 5.0], [10.0, 20.0]], dtype=torch.float64, device="cuda")
    start = torch.tensor([0, 2], dtype=torch.int32, device="cuda")
    out, counter = ops.eval_match(pred_seg, start, gt_seg, start, torch.tensor(TIOUS, dtype=torch.float64, device="cuda"))
    assert int(counter.item()) == 1 and out[:, 1].tolist() == [1] * len(TIOUS)

    ann = lambda seg, label: {"segment": seg, "label": label}
    gt = {"database": {"v0": {"subset": "test", "annotations": [ann([5.0, 5.0], names[0]), ann([10.0, 20.0], names[1])]},
                       "v1": {"subset": "test", "annotations": [ann([1.0 + 10 * k, 4.0 + 10 * k], n) for k, n in enumerate(names)]}}}
    det_row = lambda seg, label, score: {"segment": seg, "label": label, "score": score, "uncertainty": 1 - score,
                                         "actionness": score}
    results = {"v0": [det_row([5.0, 5.0], names[0], 0.9), det_row([10.0, 19.0], names[1], 0.8), det_row([30.0, 40.0], names[1], 0.7)],
               "v1": [det_row([21.0, 24.5], names[2], 0.6)]}
    local = dict(paths)
    local["gt"] = str(tmp_path / "gt.json")
    local["eval_pred.json"] = str(tmp_path / "pred.json")
    json.dump(gt, open(local["gt"], "w"))
    json.dump({"version": "x", "results": results, "external_data": {}}, open(local["eval_pred.json"], "w"))
    cuda = detector(local, "gt", openset=False, device="cuda")
    with pytest.warns(UserWarning, match="eval_match"):
        cuda.pre_evaluate()
        got_ap = cuda.evaluate(type="AP")
    cpu = detector(local, "gt", openset=False, device="cpu")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")         # numpy's own 0 / 0 warning
        cpu.pre_evaluate()
        want_ap = cpu.evaluate(type="AP")
    assert cuda.eval_data == cpu.eval_data
    assert np.array_equal(got_ap[2], want_ap[2]) and got_ap[1] == want_ap[1]
