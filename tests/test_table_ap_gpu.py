"""GPU: otal_average_precision (csrc/ap.hip) against the numpy arithmetic on hand-made codes at the workgroup tile's edges, and
table_ap (torch plumbing -> otal_eval_match -> otal_average_precision) against ap_reference on every case of
table_ap_cases.py, ties included.

Tolerance (table_ap.tolerance, derived in the module's docstring): |dAP| <= 4 npos 2^-53 with the case's own npos."""
import warnings

import numpy as np
import pytest

import table_ap_cases as cases

pytestmark = pytest.mark.gpu

ALL = cases.all_cases()


@pytest.fixture(scope="module")
def reference():
    """ap_reference of every case, computed once."""
    from opental_amd.evaluation.table_ap import ap_reference
    return {c['name']: ap_reference(c['det'], c['gt'], c['thresholds'], c['n_classes']) for c in ALL}


def _table_ap(case, pieces=1):
    import torch
    from opental_amd.evaluation.table_ap import table_ap
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message="table_ap")        # a fall-back to the CPU warns: the result must be the kernel's
        return table_ap(cases.device_tables(case, torch.device("cuda"), pieces), cases.ground_truth(case), case['thresholds'])


@pytest.mark.parametrize("case", ALL, ids=[c['name'] for c in ALL])
def test_table_ap_equals_the_reference(case, reference):
    from opental_amd.evaluation.table_ap import tolerance
    got, want = _table_ap(case), reference[case['name']]
    assert got.dtype == np.float64 and got.shape == want.shape
    tol = tolerance(cases.npos_max(case))
    err = float(np.abs(got - want).max())
    print(case['name'], "npos", cases.npos_max(case), "max |dAP|", err, "tolerance", tol)
    assert tol < 1e-12 and err <= tol
    if case['name'] == 'tied_scores':
        assert abs(got[0, 0] - cases.TIE_AP) <= tol


def test_two_calls_give_the_same_bits():
    case = next(c for c in ALL if c['name'] == 'class_sizes')
    a, b = _table_ap(case), _table_ap(case)
    assert a.tobytes() == b.tobytes() and (a > 0).any()


@pytest.mark.parametrize("name", ["class_sizes+unknown", "tied_random", "150x3"])
def test_three_batches_give_the_bits_of_one_table(name):
    case = next(c for c in ALL if c['name'] == name)
    assert _table_ap(case, pieces=3).tobytes() == _table_ap(case).tobytes()


def test_class_without_ground_truth_raises_before_any_launch():
    import torch
    from opental_amd.evaluation.table_ap import GroundTruth, table_ap
    case = ALL[0]
    gt = GroundTruth(case['gt']['video'], case['gt']['cls'], case['gt']['seg'], 3, {cases.video_name(0): 0})
    with pytest.raises(KeyError) as e:
        table_ap(cases.device_tables(case, torch.device("cuda")), gt, case['thresholds'])
    assert e.value.args == (2,)


# ------------------------------------------------------------------------------------------------ the kernel alone
def _arithmetic(codes, rank_pos, class_start, gt_count):
    """compute_average_precision_detection's tail in numpy, per class."""
    from opental_amd.evaluation.utils_eval import interpolated_prec_rec
    ap = np.zeros((codes.shape[0], len(gt_count)))
    for c in range(len(gt_count)):
        rows = rank_pos[class_start[c]:class_start[c + 1]]
        if len(rows) == 0:
            continue
        tp_cum = np.cumsum(codes[:, rows] >= 0, axis=1).astype(np.float64)
        precision = tp_cum / np.arange(1, len(rows) + 1, dtype=np.float64)
        for t in range(codes.shape[0]):
            ap[t, c] = interpolated_prec_rec(precision[t], tp_cum[t] / float(gt_count[c]))
    return ap


SIZES = cases.CLASS_SIZES + (0, 4 * cases.TILE + 5)      # + an empty class and one of five chunks (npos keeps 4 npos 2^-53 < 1e-12)


def _hand_made(seed, nthr=3, tail=0):
    """One class per size of SIZES (an empty one among them), rank_pos a random permutation of the positions, random codes;
    thresholds differ in their share of true positives, the first has none and the last has only true positives.  tail: rows
    past class_start[K] that belong to no class."""
    rs = np.random.RandomState(seed)
    class_start = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int32)
    N = int(class_start[-1]) + tail
    rank_pos = rs.permutation(N).astype(np.int32)
    share = (np.linspace(0.0, 1.0, nthr) if nthr > 1 else np.array([0.5]))[:, None]
    codes = np.where(rs.rand(nthr, N) < share, rs.randint(0, 50, (nthr, N)), rs.randint(-2, 0, (nthr, N))).astype(np.int32)
    gt_count = (np.array(SIZES) + rs.randint(0, 4, len(SIZES))).astype(np.int32)       # npos >= the true positives
    gt_count[gt_count == 0] = 1
    return codes, rank_pos, class_start, gt_count


def _dev(arrays):
    import torch
    return [torch.from_numpy(a).cuda() for a in arrays]


@pytest.mark.parametrize("nthr,tail", [(3, 0), (1, 9), (32, 0)])
def test_kernel_equals_the_arithmetic_at_the_tile_edges(nthr, tail):
    from opental_amd.common import ops
    from opental_amd.evaluation.table_ap import tolerance
    arrays = _hand_made(nthr, nthr, tail)
    want = _arithmetic(*arrays)
    got = ops.average_precision(*_dev(arrays)).cpu().numpy()
    assert got.shape == want.shape == (nthr, len(SIZES))
    tol = np.array([tolerance(n) for n in arrays[3]])[None, :]
    err = np.abs(got - want)
    print("max |dAP| per class", err.max(axis=0), "tolerance", tol[0])
    assert tol.max() < 1e-12 and (err <= tol).all()
    assert (got[:, SIZES.index(0)] == 0.0).all()            # a class without rows: written, 0
    if nthr > 1:
        assert (got[0] == 0.0).all()                        # no true positive at all
        assert (np.abs(got[-1] - np.array(SIZES) / arrays[3]) <= tol[0]).all()      # only true positives: AP = rows / npos


def test_kernel_is_bitwise_repeatable_and_writes_into_out():
    import torch
    from opental_amd.common import ops
    dev = _dev(_hand_made(5))
    out = torch.full((3, len(SIZES)), float('nan'), dtype=torch.float64, device="cuda")
    a = ops.average_precision(*dev, out=out)
    assert a is out and not torch.isnan(out).any()          # every element written
    b = ops.average_precision(*dev)
    assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


def test_no_rows_writes_zeros():
    import torch
    from opental_amd.common import ops
    z = lambda *shape: torch.zeros(shape, dtype=torch.int32, device="cuda")
    out = torch.full((2, 4), float('nan'), dtype=torch.float64, device="cuda")
    ops.average_precision(z(2, 0), z(0), z(5), z(4) + 1, out=out)
    assert (out == 0).all()


def test_refused_call_leaves_out_untouched():
    import torch
    from opental_amd.common import ops
    codes, rank_pos, class_start, gt_count = _dev(_hand_made(6, nthr=33))
    out = torch.full((33, len(SIZES)), float('nan'), dtype=torch.float64, device="cuda")
    with pytest.raises(RuntimeError, match="otal_average_precision"):
        ops.average_precision(codes, rank_pos, class_start, gt_count, out=out)         # nthr > 32
    torch.cuda.synchronize()
    assert torch.isnan(out).all()
    with pytest.raises(RuntimeError):
        ops.average_precision(codes[:3].contiguous(), rank_pos.long(), class_start, gt_count)      # dtype
    with pytest.raises(RuntimeError):
        ops.average_precision(codes[:3].contiguous(), rank_pos[:-1].contiguous(), class_start, gt_count)   # shape
