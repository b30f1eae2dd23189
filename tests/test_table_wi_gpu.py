"""GPU: otal_wilderness_impact (csrc/wi.hip) through ops.wilderness_impact against the rule's arithmetic
(table_wi.codes_reference) on every case of table_wi_cases.py, and table_wi (torch filter and sort -> otal_eval_match_labeled ->
otal_wilderness_impact) against wi_reference on device tables of the column cases, the non-finite fallback included.

Tolerance (table_wi.tolerance, derived in the module's docstring): within 4 (m + 1) 2^-53 of the rule per (threshold, class),
m = the largest number of tp_u2u rows of a threshold + 1 for a kernel case, the unknown ground truths + 1 for a table case."""
import warnings

import numpy as np
import pytest
import torch

import table_wi_cases as cases

pytestmark = pytest.mark.gpu

KERNEL_CASES = cases.kernel_cases()
DIRTY = [cases.polluted(c, i) for i, c in enumerate(KERNEL_CASES) if c['name'] in ('n775', 'u_first_row', 'class_in_last_tile')]
TABLE_CASES = cases.host_cases()


def _args(c):
    return c['codes'], c['pred_label'], c['gt_label'], c['n_known'], c['n_unknown'], c['K']


@pytest.fixture(scope="module")
def reference():
    """codes_reference of every kernel case, computed once."""
    from opental_amd.evaluation.table_wi import codes_reference
    return {c['name']: codes_reference(*_args(c)) for c in KERNEL_CASES + DIRTY}


def _device_wi(case):
    from opental_amd.common import ops
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return ops.wilderness_impact(up(case['codes']), up(case['pred_label']), up(case['gt_label']), case['n_known'],
                                 case['n_unknown'], case['K']).cpu().numpy()


def _compare(name, got, want, m):
    from opental_amd.evaluation.table_wi import tolerance
    assert got.dtype == np.float64 and got.shape == want.shape
    tol = tolerance(m)
    err = float(np.abs(got - want).max()) if got.size else 0.0
    print(name, "m", m, "max |d|", err, "tolerance", tol, "mean WI", want.mean(axis=1).tolist())
    assert tol < 1e-12 and np.isfinite(got).all() and err <= tol


@pytest.mark.parametrize("case", KERNEL_CASES, ids=[c['name'] for c in KERNEL_CASES])
def test_kernel_equals_the_rule(case, reference):
    got = _device_wi(case)
    want = reference[case['name']]
    _compare(case['name'], got, want, case['m'])
    if case['codes'].shape[1] == 0:
        assert (got == 0).all() and got.shape == (1, 15)
    elif case['codes'].shape[1] >= cases.TILE - 1 and case['name'] != 'all_predicted_unknown':
        assert (want > 0).any() and (want <= 1).all()
    if case['name'] == 'all_predicted_unknown':
        assert (got == 0).all()                 # no detection of any class: every precision ratio is 0 / 1e-6
    if case['name'] == 'class_in_last_tile':
        assert got[0, case['K'] - 1] > 0


@pytest.mark.parametrize("case", DIRTY, ids=[c['name'] for c in DIRTY])
def test_out_of_range_codes_and_labels_have_no_effect(case, reference):
    base = next(c for c in KERNEL_CASES if c['name'] + '_polluted' == case['name'])
    got = _device_wi(case)
    assert got.tobytes() == _device_wi(base).tobytes()
    assert reference[case['name']].tobytes() == reference[base['name']].tobytes()
    _compare(case['name'], got, reference[base['name']], base['m'])


def test_two_runs_give_the_same_bits():
    for name in ('n775', 'u_on_tile_edges', 'nthr32'):
        case = next(c for c in KERNEL_CASES if c['name'] == name)
        a, b = _device_wi(case), _device_wi(case)
        assert a.tobytes() == b.tobytes() and (a > 0).any()


def test_wrapper_checks_its_arguments_and_writes_into_out():
    from opental_amd.common import ops
    from opental_amd.evaluation.table_wi import codes_reference, tolerance
    codes = torch.tensor([[1, 0, 0, 2, 1, -1, -1, -2]], dtype=torch.int32, device="cuda")
    pred = torch.tensor([1, 1, 0, 1, 0, 0, 2, 1], dtype=torch.int32, device="cuda")
    gt = torch.tensor([0, 1, 2], dtype=torch.int32, device="cuda")
    out = torch.full((1, 2), 7.0, dtype=torch.float64, device="cuda")
    assert ops.wilderness_impact(codes, pred, gt, 3, 2, 2, out=out) is out
    want = codes_reference(codes.cpu().numpy(), pred.cpu().numpy(), gt.cpu().numpy(), 3, 2, 2)
    assert np.abs(out.cpu().numpy() - want).max() <= tolerance(2) and abs(want[0, 1] - 0.75) < 1e-5
    empty = ops.wilderness_impact(codes[:, :0].contiguous(), pred[:0].contiguous(), gt, 3, 2, 2)
    assert (empty.cpu().numpy() == 0).all() and tuple(empty.shape) == (1, 2)
    no_gt = ops.wilderness_impact(torch.full_like(codes, -1), pred, gt[:0].contiguous(), 3, 2, 2)      # M = 0: background only
    assert np.isfinite(no_gt.cpu().numpy()).all()
    with pytest.raises(RuntimeError, match="int32"):
        ops.wilderness_impact(codes.long(), pred, gt, 3, 2, 2)
    with pytest.raises(RuntimeError, match="pred_label"):
        ops.wilderness_impact(codes, pred[:5].contiguous(), gt, 3, 2, 2)
    with pytest.raises(RuntimeError, match="out must be"):
        ops.wilderness_impact(codes, pred, gt, 3, 2, 2, out=out[:, :1].contiguous())
    out.fill_(7.0)
    with pytest.raises(RuntimeError, match="otal_wilderness_impact"):
        ops.wilderness_impact(codes, pred, gt, 0, 2, 2, out=out)                 # no known ground truth: refused
    with pytest.raises(RuntimeError, match="otal_wilderness_impact"):
        ops.wilderness_impact(codes, pred, gt, 2 ** 24, 2, 2, out=out)           # a count the float32 rule cannot hold
    with pytest.raises(RuntimeError, match="otal_wilderness_impact"):
        ops.wilderness_impact(codes.expand(33, 8).contiguous(), pred, gt, 3, 2, 2)          # nthr > 32
    assert (out.cpu().numpy() == 7.0).all()                                      # a refused call writes nothing


# ----------------------------------------------------------------------------------------------------------- tables -> WI
def _tables(case, device="cuda", spare=5):
    """The case's detections as one device table per video (what a driver's batches give), each with `spare` rows of rubbish
    behind its n valid ones, and the ground truth as a GroundTruth numbered by the case's names."""
    from opental_amd.evaluation.table_ap import GroundTruth
    det, gt = case['det'], case['gt']
    tables = []
    for v in range(len(case['names'])):
        rows = np.nonzero(det['video'] == v)[0]
        n = len(rows)
        pad = lambda a, fill: np.concatenate((a[rows], np.full((spare,) + a.shape[1:], fill, dtype=a.dtype)))
        tables.append(dict(video=torch.from_numpy(pad(det['video'], 0)).to(device), cls=torch.from_numpy(pad(det['cls'], 1)).to(device),
                           seg=torch.from_numpy(pad(det['seg'], 3.0)).to(device), known=torch.from_numpy(pad(det['known'], 0.5)).to(device),
                           n=torch.tensor(n, device=device)))
    truth = GroundTruth(gt['video'], gt['cls'], gt['seg'], case['n_classes'], {n: v for v, n in enumerate(case['names'])})
    return tables, truth


@pytest.mark.parametrize("case", TABLE_CASES, ids=[c['name'] for c in TABLE_CASES])
def test_table_wi_equals_the_rule(case):
    from opental_amd.evaluation.table_wi import table_wi, table_wi_counted, wi_reference
    tables, truth = _tables(case)
    want = wi_reference(case['det'], case['gt'], case['thresholds'], case['ood_threshold'], n_classes=case['n_classes'],
                        video_rank=cases.rank_of(case))
    got, counter = table_wi_counted(tables, truth, case['thresholds'], case['ood_threshold'])
    assert counter == 0                                         # not the fallback
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message="table_wi")
        again = table_wi(tables, truth, case['thresholds'], case['ood_threshold'])
    assert again.tobytes() == got.tobytes()
    _compare("table_wi " + case['name'], got, want, case['m'])
    assert (want > 0).all() and (want < 1).all()
    if case['name'] == 'names_b_a_c':                           # the list order is not the evaluator's: it would show here
        by_position = wi_reference(case['det'], case['gt'], case['thresholds'], case['ood_threshold'], n_classes=case['n_classes'])
        assert np.abs(by_position - got).max() > 1e-6
    # another threshold, and none: the relabelling happens on the device
    for thr in (0.8, None):
        want = wi_reference(case['det'], case['gt'], case['thresholds'], thr, n_classes=case['n_classes'], video_rank=cases.rank_of(case))
        _compare("table_wi %s thr=%s" % (case['name'], thr), table_wi(tables, truth, case['thresholds'], thr), want, case['m'])


def test_no_detections_and_nonfinite_tiou():
    from opental_amd.evaluation.table_ap import GroundTruth
    from opental_amd.evaluation.table_wi import table_wi, table_wi_counted, wi_reference
    case = TABLE_CASES[0]
    tables, truth = _tables(case)
    for t in tables:
        t['n'] = torch.tensor(0, device="cuda")
    assert (table_wi(tables, truth, [0.3, 0.5], 0.4) == np.zeros((2, case['n_classes']))).all()
    # a zero-length detection on a zero-length ground truth: tIoU 0 / 0, the matching's counter, the rule on the CPU instead
    det = dict(video=np.zeros(3, dtype=np.int32), cls=np.array([0, 0, 1], dtype=np.int32),
               seg=np.array([[5.0, 5.0], [10.0, 20.0], [30.0, 41.0]]), known=np.array([0.75, 0.5, 0.25]))
    table = {k: torch.from_numpy(v).cuda() for k, v in det.items()}
    table['n'] = torch.tensor(3, device="cuda")
    gt = GroundTruth([0, 0, 0], [0, -1, -1], [[5.0, 5.0], [10.0, 20.0], [30.0, 40.0]], 2, {"video_0": 0})
    assert table_wi_counted([table], gt, [0.5], 0.4)[1] != 0
    with pytest.warns(UserWarning, match="table_wi"):
        got = table_wi([table], gt, [0.5], 0.4)
    want = wi_reference(det, gt.columns(), [0.5], 0.4, n_classes=2)
    assert got.tobytes() == want.tobytes() and got.shape == (1, 2)
