"""GPU: otal_eval_match_labeled (csrc/eval.hip) against match_labeled_reference -- codes and max_tiou exact -- and
ANETdetection(device='cuda').evaluate('WI') against the CPU path and the golden results of the reference."""
import warnings

import numpy as np
import pytest

from eval_match_cases import TIOUS
from eval_wi_cases import LABEL_REGIMES, edge_groups, open_detector, stats_outcome, wi_golden, wi_paths

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def paths(golden_dir):
    return wi_paths(golden_dir)


def _device_equals_reference(arrays, thresholds):
    from opental_amd.evaluation.match import match_labeled_device, match_labeled_reference
    want, want_top = match_labeled_reference(*arrays, thresholds)
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message="eval_match")      # a fall-back to the CPU warns: the codes must be the kernel's
        got, top = match_labeled_device(*arrays, thresholds)
    assert got.dtype == np.int32 and got.shape == want.shape and top.dtype == np.float64 and top.shape == want_top.shape
    assert np.array_equal(got, want), np.argwhere(got != want)[:10]
    assert np.array_equal(top, want_top), np.argwhere(top != want_top)[:10]
    return want, want_top


@pytest.fixture(scope="module", params=LABEL_REGIMES)
def groups(request):
    return request.param, edge_groups(request.param)


@pytest.mark.parametrize("nthr", [1, 10, 32])
def test_chunk_edges_label_regimes_and_threshold_counts(groups, nthr):
    from opental_amd.evaluation.match import match_reference
    regime, arrays = groups
    thresholds = [0.5] if nthr == 1 else np.linspace(0.05, 0.95, nthr)
    codes, top = _device_equals_reference(arrays, thresholds)
    ps, pl, pstart, gs, gl, gstart = arrays
    matched = codes >= 0
    assert matched.sum() > 100 and (codes == -1).any() and top.max() > 0.9
    if regime == "equal":           # every match locks: the existing rule
        assert np.array_equal(codes, match_reference(ps, pstart, gs, gstart, thresholds))
    repeats = sum(len(c[c >= 0]) - len(np.unique(c[c >= 0])) for c in codes)
    if regime == "different":       # nothing ever locks: no -2, and ground truths are matched again and again
        assert not (codes == -2).any() and repeats > 100
    if regime == "mixed":           # false positives repeat on a ground truth, true positives do not
        tp = matched & (gl[np.maximum(codes, 0)] == pl[None, :])
        assert repeats > 0 and tp.any() and (matched & ~tp).any()
        for c, m in zip(codes, tp):
            assert len(np.unique(c[m])) == int(m.sum())


def test_duplicated_ground_truths_inside_a_chunk_and_across_the_64_boundary():
    rs = np.random.RandomState(4)
    ngt = 70
    start = rs.uniform(0, 600, ngt)
    gs = np.stack([start, start + rs.uniform(2, 8, ngt)], 1)
    gs[5] = gs[3]                   # the same segment twice inside the first chunk
    gs[66] = gs[10]                 # and on both sides of the 64 boundary
    gl = np.ones(ngt, np.int32)
    gl[[5, 66]] = 2
    # label 2 on a pair: the lowest row (label 1, no lock) -- twice; label 1 locks it; label 2 then reaches its own row
    ps = np.concatenate([np.repeat(gs[[3]], 4, 0), np.repeat(gs[[10]], 4, 0)])
    pl = np.array([2, 2, 1, 2] * 2, np.int32)
    arrays = (ps, pl, np.array([0, 8], np.int32), gs, gl, np.array([0, ngt], np.int32))
    codes, top = _device_equals_reference(arrays, TIOUS)
    assert all(c.tolist() == [3, 3, 3, 5, 10, 10, 10, 66] for c in codes) and (top == 1.0).all()


def test_group_above_the_ground_truth_limit_counts_and_falls_back():
    import torch
    from opental_amd.common import ops
    from opental_amd.evaluation.match import match_labeled_device, match_labeled_reference
    rs = np.random.RandomState(5)
    ngt = 1024 + 1                  # OTAL_EVAL_MAX_GT + 1
    start = np.sort(rs.uniform(0, 5000, ngt))
    gs = np.stack([start, start + rs.uniform(1, 4, ngt)], 1)
    ps = gs[[0, ngt - 1, ngt - 1, ngt // 2]] + 0.01
    pl, gl = np.array([1, 2, 1, 1], np.int32), np.ones(ngt, np.int32)
    arrays = (ps, pl, np.array([0, 4], np.int32), gs, gl, np.array([0, ngt], np.int32))
    want, want_top = match_labeled_reference(*arrays, TIOUS)
    assert want[0].tolist() == [0, ngt - 1, ngt - 1, ngt // 2]          # the false positive left the last ground truth open
    dev = [torch.from_numpy(a).cuda() for a in arrays]
    out, top, counter = ops.eval_match_labeled(*dev, torch.tensor(TIOUS, dtype=torch.float64, device="cuda"))
    assert int(counter.item()) != 0 and bool((out == -1).all())
    with pytest.warns(UserWarning, match="eval_match_labeled"):
        got, got_top = match_labeled_device(*arrays, TIOUS)
    assert np.array_equal(got, want) and np.array_equal(got_top, want_top)


def test_group_at_the_ground_truth_limit_runs_on_the_device():
    rs = np.random.RandomState(6)
    ngt = 1024
    start = np.sort(rs.uniform(0, 5000, ngt))
    gs = np.stack([start, start + rs.uniform(1, 4, ngt)], 1)
    ps = gs[[0, ngt - 1, ngt - 1, ngt // 2]] + 0.01
    arrays = (ps, np.array([1, 2, 1, 1], np.int32), np.array([0, 4], np.int32), gs, np.ones(ngt, np.int32),
              np.array([0, ngt], np.int32))
    codes, _ = _device_equals_reference(arrays, TIOUS)
    assert codes[0].tolist() == [0, ngt - 1, ngt - 1, ngt // 2]


def test_non_finite_tiou_counts_and_falls_back():
    """A zero-length prediction on a zero-length ground truth at the same instant: tIoU = 0 / 0."""
    import torch
    from opental_amd.common import ops
    from opental_amd.evaluation.match import match_labeled_device, match_labeled_reference
    arrays = (np.array([[5.0, 5.0], [10.0, 19.0]]), np.array([1, 2], np.int32), np.array([0, 2], np.int32),
              np.array([[5.0, 5.0], [10.0, 20.0]]), np.array([1, 2], np.int32), np.array([0, 2], np.int32))
    dev = [torch.from_numpy(a).cuda() for a in arrays]
    out, top, counter = ops.eval_match_labeled(*dev, torch.tensor(TIOUS, dtype=torch.float64, device="cuda"))
    assert int(counter.item()) == 1 and out[:, 1].tolist() == [1] * len(TIOUS) and float(top[1]) == 0.9
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")         # numpy's own 0 / 0 warning
        want, want_top = match_labeled_reference(*arrays, TIOUS)
    with pytest.warns(UserWarning, match="eval_match_labeled"):
        got, got_top = match_labeled_device(*arrays, TIOUS)
    assert np.array_equal(got, want) and np.array_equal(got_top, want_top, equal_nan=True)


@pytest.mark.parametrize("case,thr", [("0.3", 0.3), ("none", None)])
def test_evaluator_on_the_device_equals_the_cpu_path_and_the_reference(paths, case, thr):
    from opental_amd.evaluation.match import WI_OUTCOMES
    want = wi_golden(paths)[case]
    cuda, cpu = open_detector(paths, ood_threshold=thr, device="cuda"), open_detector(paths, ood_threshold=thr, device="cpu")
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message="eval_match")
        got = cuda.evaluate(type="WI")
    ref = cpu.evaluate(type="WI")
    assert np.array_equal(got[0], ref[0]) and got[1] == ref[1] and np.array_equal(got[2], ref[2])
    assert sorted(cuda.stats) == sorted(cpu.stats)
    for key in cpu.stats:
        assert np.array_equal(cuda.stats[key], cpu.stats[key]), key
    assert np.array_equal(stats_outcome(cuda.stats), np.array(want["outcome"], dtype=np.int8))
    assert np.array_equal(cuda.stats["max_tious"], np.array(want["max_tious"]))
    assert np.abs(got[2] - np.array(want["wi"])).max() < 1e-12
    assert set(WI_OUTCOMES) < set(cuda.stats)


def test_set_ood_threshold_keeps_the_plan_and_its_uploads(paths):
    want = wi_golden(paths)
    det = open_detector(paths, device="cuda")
    det.pre_evaluate()                          # the split pass makes the plan and the uploads that the WI pass shares
    uploads = det._plans["split"].device
    for case, thr in (("none", None), ("0.3", 0.3), ("none", None)):
        det.set_ood_threshold(thr)
        _, _, wi = det.evaluate(type="WI")
        assert np.abs(wi - np.array(want[case]["wi"])).max() < 1e-12
        assert np.array_equal(stats_outcome(det.stats), np.array(want[case]["outcome"], dtype=np.int8))
        assert det._plans["split"].device is uploads
