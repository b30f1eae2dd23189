"""CPU: the rule of opental_amd/evaluation/table_wi.py (wi_reference) against the host evaluator
(ANETdetection(openset=True, device='cpu') + set_ood_threshold + evaluate('WI')) through the real file layout, the video order
it depends on, hand-computed literal cases of its arithmetic (codes_reference), score_checkpoints' new flags and entry rules,
and otal_wilderness_impact's argument codes.

Tolerances.  Against the host: both sides run the same matching rule and the same fp64 expressions; table_wi.tolerance(m), the
bound for two different summation orders of the m recall steps, covers them.  The literal cases restate the few terms with
Python floats in the expression order of the rule: the same bound, m counted per case."""
import ctypes
import json
import os

import numpy as np
import pytest

import table_wi_cases as cases

HOST_CASES = cases.host_cases()
KERNEL_CASES = cases.kernel_cases()


def _ids(cs):
    return [c['name'] for c in cs]


def _by_name(cs, name):
    return next(c for c in cs if c['name'] == name)


def test_case_list_covers_what_it_says():
    from opental_amd.evaluation.match import wi_outcome_codes
    T = cases.TILE
    assert T == 256 and [c['codes'].shape[1] for c in KERNEL_CASES[:6]] == [0, 1, 255, 256, 257, 3 * 256 + 7]
    assert sorted({c['K'] for c in KERNEL_CASES}) == [1, 15, 20] and sorted({c['codes'].shape[0] for c in KERNEL_CASES}) == [1, 5, 32]
    outcome = lambda c: wi_outcome_codes(c['codes'], c['pred_label'], c['gt_label'])
    big = _by_name(KERNEL_CASES, 'n775')
    assert set(np.unique(outcome(big))) == {-1, 0, 1, 2, 3, 4, 5, 6}                # every outcome and "none"
    assert outcome(_by_name(KERNEL_CASES, 'u_first_row'))[0, 0] == 0 and outcome(_by_name(KERNEL_CASES, 'u_last_row'))[0, -1] == 0
    edges = outcome(_by_name(KERNEL_CASES, 'u_on_tile_edges'))
    assert (edges[:, [T - 1, T, 2 * T, 3 * T]] == 0).all()
    last = _by_name(KERNEL_CASES, 'class_in_last_tile')
    rows = np.nonzero(last['pred_label'] == last['K'])[0]
    assert len(rows) and rows.min() >= 3 * T and (outcome(last)[0, rows] == 6).any()
    assert (_by_name(KERNEL_CASES, 'all_predicted_unknown')['pred_label'] == 0).all()
    full = _by_name(KERNEL_CASES, 'found_all')
    assert full['n_unknown'] == full['u_counts'][0] == int((outcome(full) == 0).sum()) >= 2
    for c in KERNEL_CASES:
        assert c['n_unknown'] >= max(c['u_counts'], default=0) and c['n_known'] >= 1
    dirty = cases.polluted(big)
    M, K = len(big['gt_label']), big['K']
    assert ((dirty['codes'] >= M + 2) | (dirty['codes'] < -2)).any() and ((dirty['pred_label'] > K) | (dirty['pred_label'] < 0)).any()
    assert (dirty['gt_label'][M:] > K).any() and (dirty['gt_label'][M:] < 0).any() and (dirty['codes'] == M).any()
    assert _by_name(HOST_CASES, 'names_b_a_c')['names'] == ['b', 'a', 'c']
    for c in HOST_CASES:
        assert len(set(c['det']['known'].tolist())) == len(c['det']['known'])


# ------------------------------------------------------------------------------------------------ against the host evaluator
def _host_wi(case, directory):
    from opental_amd.evaluation.eval_detection import ANETdetection
    gt_file, pred_file, cls_file = cases.write_files(case, directory)
    det = ANETdetection(ground_truth_filename=gt_file, prediction_filename=pred_file, cls_idx_detection=cls_file, subset=['test'],
                        tiou_thresholds=np.array(case['thresholds']), dataset='thumos14', openset=True, ood_threshold=None,
                        ood_scoring='uncertainty', device='cpu')
    det.set_ood_threshold(case['ood_threshold'])
    wi = det.evaluate('WI')[2]
    return wi, det


@pytest.mark.parametrize("case", HOST_CASES, ids=_ids(HOST_CASES))
def test_reference_equals_the_host_evaluator(case, tmp_path):
    from opental_amd.evaluation.table_wi import tolerance, wi_reference
    want, det = _host_wi(case, tmp_path)
    got = wi_reference(case['det'], case['gt'], case['thresholds'], case['ood_threshold'], n_classes=case['n_classes'],
                       video_rank=cases.rank_of(case))
    tol = tolerance(case['m'])
    err = float(np.abs(got - want).max())
    print(case['name'], "m", case['m'], "max err", err, "tolerance", tol, "WI", want.mean(axis=1))
    assert got.shape == want.shape == (len(case['thresholds']), case['n_classes']) and got.dtype == np.float64
    # not a comparison of nothing: unknown ground truths are found, detections are relabelled, and WI is neither 0 nor 1
    assert all(det.stats[k].sum() > 0 for k in ('tp_u2u', 'tp_k2k', 'fp_u2k', 'fp_k2k', 'fp_k2u'))
    assert (det.prediction['label'] == 0).any() and (det.prediction['label'] > 0).any()
    assert (want > 0).all() and (want < 1).all() and tol < 1e-12
    assert (np.abs(got - want) <= tol).all()


def test_host_cases_hold_what_their_names_say(tmp_path):
    from opental_amd.evaluation.utils_eval import segment_iou
    orphan, outside, tied = (_by_name(HOST_CASES, n) for n in ('orphan', 'outside_class', 'tied_tiou'))
    assert not np.isin(orphan['det']['video'], orphan['gt']['video']).all()
    assert (outside['det']['cls'] >= outside['n_classes']).sum() == 3
    _, det = _host_wi(outside, tmp_path)
    assert len(det.prediction['label']) == len(outside['det']['cls']) - 3          # the evaluator drops them, as the rule does
    seg, video = tied['gt']['seg'], tied['gt']['video']
    same = [(i, j) for i in range(len(seg)) for j in range(i + 1, min(i + 2, len(seg)))
            if video[i] == video[j] and (seg[i] == seg[j]).all()]
    assert len(same) >= 8 and all(tied['gt']['cls'][i] != tied['gt']['cls'][j] for i, j in same)
    for c in HOST_CASES:                                                             # no tIoU within 1e-3 of a threshold
        for v in np.unique(c['gt']['video']):
            g = c['gt']['seg'][c['gt']['video'] == v]
            for d in c['det']['seg'][c['det']['video'] == v]:
                assert np.abs(segment_iou(d, g)[:, None] - np.asarray(c['thresholds'])[None, :]).min() > 1e-3


def test_the_video_order_is_the_evaluators_not_the_list_position(tmp_path):
    """Videos named b, a, c in list order: the evaluator walks a, b, c.  Ignoring video_rank gives another number."""
    from opental_amd.evaluation.table_wi import tolerance, video_rank, wi_reference
    case = _by_name(HOST_CASES, 'names_b_a_c')
    rank = cases.rank_of(case)
    assert rank.tolist() == [1, 0, 2] and video_rank({'x': 0, 'y': 1}).tolist() == [0, 1]
    want, _ = _host_wi(case, tmp_path)
    args = (case['det'], case['gt'], case['thresholds'], case['ood_threshold'])
    ranked = wi_reference(*args, n_classes=case['n_classes'], video_rank=rank)
    by_position = wi_reference(*args, n_classes=case['n_classes'], video_rank=None)
    tol = tolerance(case['m'])
    assert (np.abs(ranked - want) <= tol).all()
    assert np.abs(by_position - want).max() > 1e-6 > tol


# ------------------------------------------------------------------------------------------------------------ literal cases
P1 = 1.0 / (1.0 + 1e-6)             # a precision ratio of 1 / (1 + 0 + 1e-6)


def _literal_rows(rows, n_known=3, n_unknown=2, K=2):
    """rows: (code, label of the detection) per position over the ground-truth labels [unknown, class 1, class 2]."""
    from opental_amd.evaluation.table_wi import codes_reference
    codes = np.array([[r[0] for r in rows]], dtype=np.int32).reshape(1, -1)
    return codes_reference(codes, np.array([r[1] for r in rows], dtype=np.int32), np.array([0, 1, 2], dtype=np.int32), n_known,
                           n_unknown, K)


SEVEN = [(1, 1),        # tp_k2k of class 1
         (0, 1),        # fp_u2k of class 1
         (0, 0),        # tp_u2u
         (2, 1),        # fp_k2k of class 1
         (1, 0),        # fp_k2u
         (-1, 0),       # fp_bg2u
         (-1, 2),       # fp_bg2k of class 2: counts as fp_k2k
         (-2, 1)]       # no outcome


def test_literal_one_detection_of_each_outcome():
    from opental_amd.evaluation.match import wi_outcome_codes
    from opental_amd.evaluation.table_wi import tolerance
    outcome = wi_outcome_codes(np.array([[r[0] for r in SEVEN]]), np.array([r[1] for r in SEVEN]), np.array([0, 1, 2]))
    assert outcome.tolist() == [[1, 2, 0, 3, 4, 5, 6, -1]]
    got = _literal_rows(SEVEN)
    # class 1: A = 1 1 1 2 .., F = 0 1 1 1 ..: precision 1/(1+1e-6), 1/(2+1e-6), 1/(2+1e-6), 2/(3+1e-6) ..; the envelope is the
    # first value at row 0 and 2/(3+1e-6) behind it.  Recall 3/5 up to row 1, 3/4 from the tp_u2u at row 2 on.
    want1 = (3.0 / 5.0) * P1 + (3.0 / 4.0 - 3.0 / 5.0) * (2.0 / (3.0 + 1e-6))
    # class 2: A = 0 .. 0 1 1: precision 0 up to row 5 and 1/(1+1e-6) behind: the envelope is that value everywhere
    want2 = (3.0 / 5.0) * P1 + (3.0 / 4.0 - 3.0 / 5.0) * P1
    assert got.shape == (1, 2) and np.abs(got - [[want1, want2]]).max() <= tolerance(2)
    assert abs(want1 - 0.7) < 1e-5 and abs(want2 - 0.75) < 1e-5


def test_literal_edges():
    from opental_amd.evaluation.table_wi import codes_reference, tolerance, wi_reference
    # N = 0: interpolated_prec_rec of empty curves is (1 - 0) * 0
    empty = codes_reference(np.zeros((3, 0), dtype=np.int32), np.zeros(0, dtype=np.int32), np.array([0, 1], dtype=np.int32), 1, 1, 4)
    assert empty.shape == (3, 4) and (empty == 0).all() and empty.dtype == np.float64
    # no tp_u2u at all: one term, recall 3/5 times the largest precision (class 1: rows tp, fp_u2k -> 1/(1+1e-6) at row 0)
    got = _literal_rows([(1, 1), (0, 1), (-1, 2), (1, 0)])
    assert np.abs(got - [[0.6 * P1, 0.6 * P1]]).max() <= tolerance(1)
    # every unknown ground truth found: the recall ratio reaches exactly 1 and the closing step does not exist
    got = _literal_rows([(1, 1), (0, 0), (0, 1)], n_known=3, n_unknown=1)
    # class 1: A = 1 1 1, F = 0 0 1: precision P1, P1, 1/(2+1e-6); recall 3/4, 3/3, 3/3
    assert 3.0 / (3.0 + 1.0 - 1.0) == 1.0
    assert abs(got[0, 0] - (0.75 * P1 + (1.0 - 0.75) * P1)) <= tolerance(2)
    # a class without detections: precision 0 / 1e-6 = 0 everywhere, WI exactly 0 (class 2 here, and class 3 of a wider index)
    assert got[0, 1] == 0.0
    wide = codes_reference(np.array([[1, 0]], dtype=np.int32), np.array([1, 0], dtype=np.int32), np.array([0, 1, 2], dtype=np.int32),
                           3, 2, 3)
    assert wide[0, 0] > 0 and wide[0, 1] == 0.0 and wide[0, 2] == 0.0
    # through the whole rule: no detection at all, and only detections of a video without ground truth
    gt = dict(video=np.zeros(2, dtype=np.int32), cls=np.array([0, -1], dtype=np.int32), seg=np.array([[0.0, 10.0], [20.0, 30.0]]))
    none = dict(video=np.zeros(0, dtype=np.int32), cls=np.zeros(0, dtype=np.int32), seg=np.zeros((0, 2)), known=np.zeros(0))
    assert (wi_reference(none, gt, [0.3, 0.5], 0.5, n_classes=2) == np.zeros((2, 2))).all()
    orphan = dict(video=np.ones(1, dtype=np.int32), cls=np.zeros(1, dtype=np.int32), seg=np.array([[0.0, 10.0]]), known=np.array([0.9]))
    assert (wi_reference(orphan, gt, [0.5], 0.5, n_classes=2) == 0).all()
    # one detection on the known ground truth, kept known (ood 0.1 is not below 0.05), then relabelled (0.1 < 0.5: fp_k2u)
    det = dict(video=np.zeros(1, dtype=np.int32), cls=np.zeros(1, dtype=np.int32), seg=np.array([[0.0, 10.0]]), known=np.array([0.9]))
    assert abs(wi_reference(det, gt, [0.5], 0.05, n_classes=2)[0, 0] - 0.5 * P1) <= tolerance(1)
    assert wi_reference(det, gt, [0.5], 0.5, n_classes=2)[0, 0] == 0.0
    assert wi_reference(det, gt, [0.5], None, n_classes=2)[0, 0] == wi_reference(det, gt, [0.5], 0.05, n_classes=2)[0, 0]


def test_out_of_range_rows_have_no_outcome():
    from opental_amd.evaluation.table_wi import codes_reference
    base = _by_name(KERNEL_CASES, 'n775')
    dirty = cases.polluted(base)
    args = lambda c: (c['codes'], c['pred_label'], c['gt_label'], c['n_known'], c['n_unknown'], c['K'])
    assert np.array_equal(codes_reference(*args(base)), codes_reference(*args(dirty)))
    # and a row that HAS an outcome loses it: an out-of-range label on the first tp_u2u changes the recall steps
    hurt = dict(base, pred_label=base['pred_label'].copy())
    first = np.nonzero((base['pred_label'] == 0) & (base['codes'][0] >= 0) & (base['gt_label'][np.maximum(base['codes'][0], 0)] == 0))[0][0]
    hurt['pred_label'][first] = base['K'] + 1
    assert not np.array_equal(codes_reference(*args(base)), codes_reference(*args(hurt)))


def test_refusals():
    from opental_amd.evaluation.table_ap import GroundTruth
    from opental_amd.evaluation.table_wi import gt_totals, table_wi, wi_reference
    det = dict(video=np.zeros(1, dtype=np.int32), cls=np.zeros(1, dtype=np.int32), seg=np.array([[0.0, 10.0]]), known=np.array([0.9]))
    only_unknown = dict(video=np.zeros(2, dtype=np.int32), cls=np.array([-1, -1], dtype=np.int32), seg=np.array([[0.0, 10.0], [20.0, 30.0]]))
    with pytest.raises(ValueError, match="known class"):
        wi_reference(det, only_unknown, [0.5], 0.5, n_classes=2)
    with pytest.raises(ValueError, match="known class"):
        wi_reference(det, dict(video=np.zeros(0, dtype=np.int32), cls=np.zeros(0, dtype=np.int32), seg=np.zeros((0, 2))), [0.5], 0.5, n_classes=2)
    assert gt_totals(np.array([0, 1, 1, 2]), 2) == (3, 1)
    with pytest.raises(AssertionError, match="2\\^24"):
        gt_totals(np.ones(2 ** 24, dtype=np.int8), 1)
    # the device path refuses the same ground truth before it touches a table, and needs no device for no detections
    gt = GroundTruth([0, 0], [-1, -1], only_unknown['seg'], 2, {'a': 0})
    with pytest.raises(ValueError, match="known class"):
        table_wi([], gt, [0.5], 0.5)
    gt = GroundTruth([0, 0], [0, -1], only_unknown['seg'], 2, {'a': 0})
    assert (table_wi([], gt, [0.3, 0.5], 0.5) == np.zeros((2, 2))).all()
    with pytest.raises(ValueError, match="thresholds"):
        table_wi([], gt, np.linspace(0, 1, 33), 0.5)


# -------------------------------------------------------------------------------------------------------- the driver's flags
def _argv(*extra):
    return ['no_such.yaml', '--gt', 'gt.json', '--known', 'known.txt'] + list(extra)


OPEN = ('--open_set', '--open_metrics')


def test_new_flags_and_their_refusals_come_before_any_gpu_work(monkeypatch):
    from opental_amd.common import score_checkpoints as S
    monkeypatch.setattr(S, "device_setup", lambda *a: pytest.fail("a refused command line must not initialise the device"))
    refused = lambda *extra: pytest.raises(SystemExit, match=extra[-1])
    with refused("open_metrics"):
        S.run(None, _argv('--open_set', '--threshold_from_train'))
    with refused("open_metrics"):
        S.run(None, _argv('--open_set', '--wi', '--ood_threshold', '0.5'))
    with refused("open_metrics"):
        S.run(None, _argv('--open_set', '--wi'))
    with refused("exclude"):
        S.run(None, _argv(*OPEN, '--threshold_from_train', '--ood_threshold', '0.5'))
    with refused("threshold_from_train"):
        S.run(None, _argv(*OPEN, '--threshold_videos', '4'))
    with refused("threshold_from_train"):
        S.run(None, _argv(*OPEN, '--ood_threshold', '0.5', '--threshold_videos', '4'))
    with refused("positive"):
        S.run(None, _argv(*OPEN, '--threshold_from_train', '--threshold_videos', '0'))
    with refused("needs a threshold"):
        S.run(None, _argv(*OPEN, '--wi'))
    with refused("--wi"):
        S.run(None, _argv(*OPEN, '--select', 'WI', '--ood_threshold', '0.5'))
    with refused("--wi"):
        S.run(None, _argv('--select', 'WI'))
    # a recipe that cannot list its training videos
    plain = S.Recipe('thumos14', ['test'], [0.5], None, None, None, None)
    assert plain.train_videos is None and plain.train_table is None
    with refused("training videos"):
        S.run(plain, _argv(*OPEN, '--threshold_from_train'))
    own, rest = S.parse_own(_argv(*OPEN, '--threshold_from_train', '--threshold_videos', '3', '--wi', '--select', 'WI', '--split', '1'))
    assert own['--threshold_from_train'] and own['--wi'] and own['--threshold_videos'] == 3 and own['--select'] == 'WI'
    assert own['--ood_threshold'] is None and rest == ['no_such.yaml', '--open_set', '--split', '1']
    own, _ = S.parse_own(_argv(*OPEN, '--wi', '--ood_threshold', '0.25'))
    assert own['--wi'] and own['--ood_threshold'] == 0.25 and not own['--threshold_from_train'] and own['--threshold_videos'] is None
    # an old command line parses as before
    own, rest = S.parse_own(_argv('--open_set', '--open_metrics', '--select', 'FAR95', '--ood_threshold', '0.25'))
    assert own['--select'] == 'FAR95' and own['--ood_threshold'] == 0.25 and not own['--wi'] and not own['--threshold_from_train']
    own, _ = S.parse_own(_argv())
    assert not own['--open_metrics'] and not own['--wi'] and not own['--threshold_from_train'] and own['--threshold_videos'] is None


def test_both_recipes_list_their_training_split():
    from opental_amd.anet import score_checkpoints as A
    from opental_amd.thumos14 import score_checkpoints as T
    for recipe in (A.RECIPE, T.RECIPE):
        assert callable(recipe.train_videos) and callable(recipe.train_table)
    assert A._batches(None, (list(range(10)), {})) == [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9]]
    assert A._batches(None, (list(range(10)), {}, 8)) == [list(range(8)), [8, 9]]


def test_entry_and_merge_rules():
    from opental_amd.common import score_checkpoints as S
    metrics = dict(auroc=np.array([0.25, 0.5]), aupr=np.array([1.0, 0.0]), far95=np.array([np.nan, 0.125]), osdr=np.array([0.5, 0.5]))
    four = {"AUROC": [0.25, 0.5], "AUPR": [1.0, 0.0], "FAR95": [None, 0.125], "OSDR": [0.5, 0.5]}
    wi = np.array([[0.5, 0.25, 0.75], [np.nan, 0.5, 0.5]])
    # old calls give old entries
    assert S.open_entry(metrics, None) == four and S.open_entry(metrics, 0.25) == dict(four, ood_threshold=0.25)
    # the new keys
    assert S.open_entry(metrics, 0.25, wi) == dict(four, ood_threshold=0.25, WI=[0.5, None])
    train = S.open_entry(metrics, 0.3, wi, from_train=True)
    assert train == dict(four, ood_threshold=0.3, ood_threshold_from='train', WI=[0.5, None])
    capped = S.open_entry(metrics, 0.3, None, from_train=True, threshold_videos=4)
    assert capped == dict(four, ood_threshold=0.3, ood_threshold_from='train', threshold_videos=4)
    assert json.loads(json.dumps(train))['WI'] == [0.5, None]
    base = {"mAP": [0.1], "average_mAP": 0.1}
    typed, own, own4 = dict(base, **S.open_entry(metrics, 0.25)), dict(base, **train), dict(base, **capped)
    # what is held: old calls on old entries as before
    assert S.holds(typed, True, 0.25) and not S.holds(typed, True, None) and S.holds(typed, False, None)
    assert not S.holds(typed, True, 0.25, wi=True) and S.holds(dict(typed, WI=[0.1]), True, 0.25, wi=True)
    assert not S.holds(typed, True, None, from_train=True)                          # a typed threshold is not the epoch's own
    assert S.holds(own, True, None, wi=True, from_train=True) and S.holds(own, True, None, from_train=True)
    assert not S.holds(own, True, None, from_train=True, threshold_videos=4)        # made without a cap
    assert S.holds(own4, True, None, from_train=True, threshold_videos=4)
    assert not S.holds(own4, True, None, from_train=True, threshold_videos=5) and not S.holds(own4, True, None, from_train=True)
    assert not S.holds(own4, True, None, wi=True, from_train=True, threshold_videos=4)
    assert not S.holds(own, True, 0.3) and not S.holds(own, True, None)             # an own threshold is not a typed one
    assert S.holds(own, False, None)
    # merging: whatever belongs to the old threshold leaves with it
    merged = S.merge_entry(own4, dict(base, **S.open_entry(metrics, None)))
    assert merged == dict(base, **four)
    merged = S.merge_entry(dict(own, threshold_videos=2), dict(base, **S.open_entry(metrics, 0.5)))
    assert merged == dict(base, ood_threshold=0.5, **four)
    assert S.merge_entry(own, {"mAP": [0.2], "average_mAP": 0.2}) == dict({"mAP": [0.2], "average_mAP": 0.2}, **four)
    assert S.merge_entry(typed, own4) == own4
    # --select WI: the mean over the thresholds, lower is better, a null never, equal means to the earlier epoch
    scores = {'1': dict(base, WI=[0.5, 0.3]), '2': dict(base, WI=[0.2, None]), '3': dict(base, WI=[0.3, 0.1]),
              '4': dict(base, WI=[0.1, 0.3]), '5': base}
    assert 'WI' in S.SELECT_KEYS and S.best_epoch(scores, 'WI') == 3 and S.select_value(scores['1'], 'WI') == -0.4
    assert S.best_epoch({'5': base}, 'WI') is None and S.best_epoch(scores) == 1
    assert S.capped([[0, 1, 2], [3, 4, 5], [6]], 4) == [[0, 1, 2], [3]] and S.capped([[0, 1]], None) == [[0, 1]]


# ------------------------------------------------------------------------------------------------------------------- the ABI
def test_wilderness_impact_is_exported_and_its_argument_errors_do_not_launch():
    from opental_amd.common import ops
    from opental_amd.csrc import build
    if not os.path.exists(build.LIB):
        build.build(verbose=False)
    from opental_amd._lib import declare, signatures
    lib = declare(ctypes.CDLL(build.LIB))
    assert hasattr(lib, 'otal_wilderness_impact') and lib.otal_abi_version() == 26
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "opental_hip.h")).read()
    assert ("int otal_wilderness_impact(const int* codes, const int* pred_label, const int* gt_label, int n_known, int n_unknown, "
            "int N,\n                           int M, int nthr, int K, double* out, void* stream);") in header
    assert "#define OTAL_WI_MAX_GT 16777216" in header and ops.WI_MAX_GT == 16777216
    restype, argtypes = signatures()['otal_wilderness_impact']
    assert restype is ctypes.c_int and argtypes == [ctypes.c_void_p] * 3 + [ctypes.c_int] * 6 + [ctypes.c_void_p] * 2
    one = ctypes.c_void_p(16)       # never dereferenced: argument checks come first
    f = lib.otal_wilderness_impact
    good = [one, one, one, 5, 3, 10, 4, 5, 20, one, None]
    for k in (0, 1, 2, 9):                                                  # every pointer argument in turn
        args = list(good)
        args[k] = None
        assert f(*args) == -1, k                                            # OTAL_E_NULL
    for k, bad in ((3, 0), (4, -1), (5, -1), (6, -1), (7, 0), (8, 0)):      # n_known < 1, n_unknown < 0, N < 0, M < 0, nthr < 1, K < 1
        args = list(good)
        args[k] = bad
        assert f(*args) == -2, k                                            # OTAL_E_SHAPE
    for k, bad in ((7, 33), (5, ops.AP_MAX_CLASS_ROWS + 1), (3, 2 ** 24), (4, 2 ** 24 - 5)):
        args = list(good)
        args[k] = bad
        assert f(*args) == -7, k                                            # OTAL_E_UNSUPPORTED
    args = list(good)
    args[0], args[7] = None, 33
    assert f(*args) == -1                                                   # the null check comes first
