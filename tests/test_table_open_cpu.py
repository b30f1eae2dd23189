"""CPU: the rule of opental_amd/evaluation/table_open.py (open_reference) against the host evaluator
(ANETdetection(openset=True): pre_evaluate -> evaluate('AUC'), evaluate('OSDR')) through the real file layout; its degenerate
lists; its tie cases against a literal restatement in loops over groups and cuts; score_checkpoints' new flags and the merge
rules of checkpoint_map.json; and otal_open_set_curves' argument codes.

Tolerances.  Against the host: both sides are fp64 values no further apart than table_open.tolerance(n) before the host stores
float32, so the rule's value cast to float32 is within one float32 ulp of the host's; FAR@95 is equal after the same cast.
Against the literal restatement, which is exact (fractions): a term of the rule carries at most four roundings of values <= 2
and the sum n more, so |rule - exact| <= 8 (n + 2) 2^-53."""
import ctypes
import json
import os
from fractions import Fraction

import numpy as np
import pytest

import table_open_cases as cases

KERNEL_CASES = cases.kernel_cases()
HOST_CASES = cases.host_cases()


def _ids(cs):
    return [c['name'] for c in cs]


def _by_name(name):
    return next(c for c in KERNEL_CASES if c['name'] == name)


def test_case_list_covers_what_it_says():
    sizes = [c['n'] for c in KERNEL_CASES if c['name'].startswith('n') and c['name'][1:].isdigit()]
    assert sizes == [0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 513] and cases.TILE == 256
    assert sorted({c['codes'].shape[0] for c in KERNEL_CASES}) == [1, 5, 32]
    assert {c['ood_threshold'] for c in KERNEL_CASES} == {None, 0.75, 0.8}
    for c in KERNEL_CASES:
        codes = c['codes'][0]
        assert (codes == -1).any() and (codes == -2).any() and (codes >= 0).sum() == c['n']
        assert (c['gt_cls'] == -1).sum() >= c['list'][1].sum() and len(c['gt_cls']) > c['n']     # slots that stay empty
    gap = _by_name('gap')['codes'][0]
    run = max(len(r) for r in ''.join('f' if x >= 0 else 'b' for x in gap).split('f'))
    assert run >= cases.TILE                                    # a tile-sized stretch without a foreground row
    known = _by_name('tie_over_wave_edge')['list'][0]
    assert len(set(known[60:71])) == 1 and known[59] < known[60] and known[71] > known[70]
    known = _by_name('tie_over_chunk_edge')['list'][0]
    assert len(set(known[250:263])) == 1 and known[249] < known[250] and known[263] > known[262]
    assert len(set(_by_name('all_equal')['list'][0])) == 1
    assert not _by_name('only_known')['list'][1].any() and _by_name('only_unknown')['list'][1].all()
    relabel = _by_name('relabel')
    before, after = relabel['list'][2], cases.expected_flags(relabel)[2]
    assert before.sum() > after.sum() > 0                      # some correct rows are relabelled, not all
    for c in HOST_CASES:
        assert len(set(c['det']['known'].tolist())) == len(c['det']['known'])
        assert np.array_equal(c['det']['known'] * 2.0 ** 20, np.round(c['det']['known'] * 2.0 ** 20))


# ------------------------------------------------------------------------------------------------ against the host evaluator
def _host_metrics(case, directory, ood_threshold=None):
    from opental_amd.evaluation.eval_detection import ANETdetection
    gt_file, pred_file, cls_file = cases.write_files(case, directory)
    det = ANETdetection(ground_truth_filename=gt_file, prediction_filename=pred_file, cls_idx_detection=cls_file, subset=['test'],
                        tiou_thresholds=np.array(case['thresholds']), dataset='thumos14', openset=True,
                        ood_threshold=ood_threshold, ood_scoring='uncertainty', device='cpu')
    det.pre_evaluate()
    auroc, aupr, far = det.evaluate('AUC')
    osdr = det.evaluate('OSDR')
    sizes = [len(s['known']) + len(s['unknown']) for s in det.eval_data[0]]
    kinds = [(len(s['known']), len(s['unknown'])) for s in det.eval_data[0]]
    return dict(auroc=auroc, aupr=aupr, far95=far, osdr=osdr), sizes, kinds


def _check_against_host(got, want, sizes):
    from opental_amd.evaluation.table_open import tolerance
    for key in ('auroc', 'aupr', 'osdr'):
        assert got[key].dtype == np.float64 and want[key].dtype == np.float32
        ulp = np.spacing(np.abs(want[key]))
        err = np.abs(got[key].astype(np.float32) - want[key])
        print(key, "sizes", sizes, "max err", float(err.max()), "ulp", float(ulp.max()), "tolerance", tolerance(max(sizes)))
        assert tolerance(max(sizes)) < 2.0 ** -30 and (err <= ulp).all(), key
    assert np.array_equal(got['far95'].astype(np.float32), want['far95'], equal_nan=True)


@pytest.mark.parametrize("case", HOST_CASES, ids=_ids(HOST_CASES))
@pytest.mark.parametrize("relabel", [False, True])
def test_reference_equals_the_host_evaluator(case, relabel, tmp_path):
    from opental_amd.evaluation.table_open import open_reference
    ood_threshold = 0.4 if relabel else None
    want, sizes, kinds = _host_metrics(case, tmp_path, ood_threshold)
    got = open_reference(case['det'], case['gt'], case['thresholds'], ood_threshold, n_classes=case['n_classes'])
    assert min(min(k) for k in kinds) > 0 and (want['auroc'] > 0).all()         # both kinds matched at every threshold
    _check_against_host(got, want, sizes)
    if relabel:
        plain = open_reference(case['det'], case['gt'], case['thresholds'], None, n_classes=case['n_classes'])
        assert (got['osdr'] < plain['osdr']).any() and np.array_equal(got['auroc'], plain['auroc'])


# --------------------------------------------------------------------------------------------------------- degenerate lists
def test_degenerate_lists():
    from opental_amd.evaluation.table_open import curves_reference, open_reference
    e = np.zeros(0)
    assert curves_reference(e, e, e.astype(bool), e.astype(bool)) == (0.0, 0.0, 0.0, 0.0)
    one = np.array([0.25])
    for unknown, correct in ((False, True), (False, False), (True, False)):
        out = curves_reference(one, np.zeros(1, dtype=int), np.array([correct]), np.array([unknown]))
        assert out[3] == 0.5 and out[0] == 0.0                  # n = 1: OSDR 0.5 whatever the entry
    known = (1.0 + np.arange(6)) / 8.0
    rows = np.arange(6)
    none, every = np.zeros(6, dtype=bool), np.ones(6, dtype=bool)
    auroc, aupr, far, osdr = curves_reference(known, rows, every, none)          # no unknown matched
    assert (auroc, aupr, far) == (0.0, 0.0, 0.0) and osdr > 0
    auroc, aupr, far, osdr = curves_reference(known, rows, none, every)          # no known matched
    assert auroc == 0.0 and aupr == 1.0 and far != far
    # through the whole rule: no detection matches, and a video without ground truth is dropped
    det = dict(video=np.array([0, 1], dtype=np.int32), cls=np.zeros(2, dtype=np.int32), seg=np.array([[50.0, 60.0], [0.0, 10.0]]),
               known=np.array([0.5, 0.25]))
    gt = dict(video=np.zeros(1, dtype=np.int32), cls=np.zeros(1, dtype=np.int32), seg=np.array([[0.0, 10.0]]))
    out = open_reference(det, gt, [0.3, 0.5])
    assert all((out[k] == 0).all() and out[k].shape == (2,) and out[k].dtype == np.float64 for k in out)
    assert sorted(out) == ['aupr', 'auroc', 'far95', 'osdr']
    det['video'][1] = 0                                         # now it matches: one known entry
    out = open_reference(det, gt, [0.3, 0.5])
    assert (out['osdr'] == 0.5).all() and (out['far95'] == 0).all()
    out = open_reference(det, gt, [0.3, 0.5], n_classes=0)      # every class is outside the index
    assert (out['osdr'] == 0).all()


def test_twenty_tied_pairs_keep_two_points():
    from opental_amd.evaluation.table_open import codes_reference
    c = _by_name('pairs20')
    out = codes_reference(c['codes'], c['row'], c['known'], c['cls'], c['gt_cls'])
    assert out[0, 2] == 1.0                                     # the full curve would give 0.95


# ------------------------------------------------------------------------------------------------- the literal restatement
def _literal(known, unknown, correct):
    """(AUROC, AUPR, FAR@95, OSDR) of one list in (known, row) order, by loops: the first three exact."""
    n = len(known)
    if n == 0:
        return 0.0, 0.0, 0.0, 0.0
    P = sum(bool(u) for u in unknown)
    Q = n - P
    # tie groups by descending ood = ascending known; (fps, tps) at every group's end
    points, tps, fps = [], 0, 0
    for i in range(n):
        tps, fps = tps + bool(unknown[i]), fps + (not unknown[i])
        if i == n - 1 or (1.0 - known[i + 1]) != (1.0 - known[i]):
            points.append((fps, tps))
    aupr, last = Fraction(0), Fraction(0)
    for f, t in points:
        recall = Fraction(t, P) if P else Fraction(1)
        aupr += (recall - last) * Fraction(t, t + f)
        last = recall
    kept = [p for g, p in enumerate(points) if g in (0, len(points) - 1)
            or points[g][0] - points[g - 1][0] != points[g + 1][0] - points[g][0]
            or points[g][1] - points[g - 1][1] != points[g + 1][1] - points[g][1]]
    curve = [(0, 0)] + kept
    auroc = Fraction(0)
    if P and Q:
        for (f0, t0), (f1, t1) in zip(curve[:-1], curve[1:]):
            auroc += Fraction(f1 - f0, Q) * (Fraction(t1, P) + Fraction(t0, P)) / 2
    if P == 0:
        far = 0.0
    elif Q == 0:
        far = float('nan')
    else:
        best = None
        for f, t in curve:
            d = abs(float(t) / float(P) - 0.95)
            if best is None or d < best[0]:
                best = (d, float(f) / float(Q))
        far = best[1]
    # OSDR: one point per cut, the reference's sorted(zip(FPR, CCR), reverse=True), trapezoids
    pts = [(Fraction(1), Fraction(1)), (Fraction(0), Fraction(0)), (Fraction(0), Fraction(0))]
    for k in range(n - 1):
        above_correct = sum(bool(correct[i]) and not unknown[i] for i in range(k + 1, n))
        at_or_above_unknown = sum(bool(unknown[i]) for i in range(k, n))
        pts.append((Fraction(at_or_above_unknown, P) if P else Fraction(0), Fraction(above_correct, Q) if Q else Fraction(1)))
    pts.sort(reverse=True)
    osdr = sum(((f0 - f1) * (c0 + c1) / 2 for (f0, c0), (f1, c1) in zip(pts[:-1], pts[1:])), Fraction(0))
    return float(auroc), float(aupr), far, float(osdr)


TIE_CASES = [c for c in KERNEL_CASES if c['name'] in ('all_equal', 'tie_over_wave_edge', 'tie_over_chunk_edge', 'pairs20',
                                                      'collinear_tail', 'alternating', 'relabel_ties', 'n3', 'n65')]


@pytest.mark.parametrize("case", TIE_CASES, ids=_ids(TIE_CASES))
def test_tie_cases_equal_a_literal_restatement(case):
    from opental_amd.evaluation.table_open import codes_reference
    got = codes_reference(case['codes'], case['row'], case['known'], case['cls'], case['gt_cls'], case['ood_threshold'])
    for t in range(min(got.shape[0], 3)):
        known, unknown, correct = cases.expected_flags(case, t)
        want = _literal(known.tolist(), unknown.tolist(), correct.tolist())
        tol = 8.0 * (len(known) + 2) * 2.0 ** -53
        print(case['name'], t, got[t], want)
        for k in (0, 1, 3):
            assert abs(got[t, k] - want[k]) <= tol, (t, k)
        assert got[t, 2] == want[2] or (got[t, 2] != got[t, 2] and want[2] != want[2])


def test_equal_known_goes_by_table_row():
    from opental_amd.evaluation.table_open import osdr_reference
    known = np.array([0.5, 0.5, 0.5, 0.75])
    unknown = np.array([True, False, False, False])
    correct = np.array([False, True, True, True])
    a = osdr_reference(known, np.array([0, 1, 2, 3]), correct, unknown)            # the unknown first in the tie
    b = osdr_reference(known, np.array([2, 0, 1, 3]), correct, unknown)            # the unknown last in the tie
    tol = 8.0 * 6 * 2.0 ** -53                                  # the restatement is exact: the module docstring's bound, n = 4
    assert abs(a - _literal(known.tolist(), unknown.tolist(), correct.tolist())[3]) <= tol and abs(a - b) > 0.01
    assert abs(b - _literal(known.tolist(), [False, False, True, False], [True, True, False, True])[3]) <= tol


# -------------------------------------------------------------------------------------------------------- the driver's flags
def _argv(*extra):
    return ['no_such.yaml', '--gt', 'gt.json', '--known', 'known.txt'] + list(extra)


def test_flag_parsing():
    from opental_amd.common import score_checkpoints as S
    with pytest.raises(SystemExit, match="open_metrics"):
        S.run(None, _argv('--open_set', '--select', 'AUROC'))          # a key that is not scored
    with pytest.raises(SystemExit, match="open_metrics"):
        S.run(None, _argv('--open_set', '--ood_threshold', '0.5'))
    with pytest.raises(SystemExit, match="open_set"):
        S.run(None, _argv('--open_metrics'))
    with pytest.raises(SystemExit, match="select"):
        S.run(None, _argv('--open_set', '--open_metrics', '--select', 'mAP'))
    own, rest = S.parse_own(_argv('--open_set', '--open_metrics', '--select', 'FAR95', '--ood_threshold', '0.25', '--split', '1'))
    assert own['--open_metrics'] and own['--select'] == 'FAR95' and own['--ood_threshold'] == 0.25
    assert rest == ['no_such.yaml', '--open_set', '--split', '1']
    own, rest = S.parse_own(_argv())
    assert not own['--open_metrics'] and own['--select'] == 'average_mAP' and own['--ood_threshold'] is None


def test_file_merge_rules(tmp_path):
    from opental_amd.common import score_checkpoints as S
    from opental_amd.common.driver import write_json
    full = lambda far, osdr: {"mAP": [0.1], "average_mAP": 0.1, "AUROC": [0.5, 0.5], "AUPR": [0.4, 0.4], "FAR95": far, "OSDR": osdr}
    path = str(tmp_path / S.MAP_FILE)
    written = {"1": {"mAP": [0.3, 0.1], "average_mAP": 0.2}, "2": full([0.9, None], [0.2, 0.2]), "3": full([0.5, 0.7], [0.3, 0.1]),
               "4": dict(full([0.7, 0.5], [0.1, 0.3]), ood_threshold=0.25), "best": 1}
    with open(path, "w") as f:
        json.dump(written, f)
    scores = S.read_map(path)
    assert sorted(scores) == ['1', '2', '3', '4']
    # what is skipped: an entry that holds everything asked for
    assert S.holds(scores['1'], False, None) and not S.holds(scores['1'], True, None)
    assert S.holds(scores['3'], True, None) and not S.holds(scores['3'], True, 0.25)
    assert S.holds(scores['4'], True, 0.25) and not S.holds(scores['4'], True, None) and S.holds(scores['4'], False, None)
    assert not S.holds({"AUROC": [1.0]}, False, None)
    # what is best: the mean over the thresholds; lower for FAR95; a NaN mean never; equal means go to the earlier epoch; an
    # epoch without the key never
    assert S.best_epoch(scores) == 1 and S.best_epoch(scores, 'average_mAP') == 1
    assert S.best_epoch(scores, 'FAR95') == 3                   # 2: NaN; 3 and 4: 0.6
    assert S.best_epoch(scores, 'OSDR') == 2 and S.best_epoch(scores, 'AUROC') == 2
    assert S.best_epoch({'1': scores['1']}, 'AUROC') is None and S.best_epoch({}) is None
    assert S.select_value(scores['3'], 'FAR95') == -0.6 and S.select_value(scores['2'], 'FAR95') != S.select_value(scores['2'], 'FAR95')
    # merging: the old keys stay, the new ones win, an ood_threshold only where the new scoring had one
    new = S.open_entry(dict(auroc=np.array([0.25, 0.5]), aupr=np.array([1.0, 0.0]), far95=np.array([np.nan, 0.125]),
                            osdr=np.array([0.5, 0.5])), None)
    assert new == {"AUROC": [0.25, 0.5], "AUPR": [1.0, 0.0], "FAR95": [None, 0.125], "OSDR": [0.5, 0.5]}
    merged = S.merge_entry(scores['4'], dict({"mAP": [0.2], "average_mAP": 0.2}, **new))
    assert 'ood_threshold' not in merged and merged['mAP'] == [0.2] and merged['FAR95'] == [None, 0.125]
    assert S.merge_entry(scores['1'], S.open_entry(dict(auroc=[0.5], aupr=[0.5], far95=[0.5], osdr=[0.5]), 0.25)) == \
        {"mAP": [0.3, 0.1], "average_mAP": 0.2, "AUROC": [0.5], "AUPR": [0.5], "FAR95": [0.5], "OSDR": [0.5], "ood_threshold": 0.25}
    assert S.merge_entry(None, {"mAP": [1.0]}) == {"mAP": [1.0]}
    write_json(path, dict(scores, **{"4": merged, "best": S.best_epoch(scores, 'FAR95')}))
    text = open(path).read()
    assert 'NaN' not in text and '[null, 0.125]' in text and json.loads(text)['best'] == 3


# ------------------------------------------------------------------------------------------------------------------- the ABI
def test_open_set_curves_is_exported_and_its_argument_errors_do_not_launch():
    from opental_amd.common import ops
    from opental_amd.csrc import build
    if not os.path.exists(build.LIB):
        build.build(verbose=False)
    from opental_amd._lib import declare
    lib = declare(ctypes.CDLL(build.LIB))
    assert hasattr(lib, 'otal_open_set_curves') and lib.otal_abi_version() == 26
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "opental_hip.h")).read()
    assert "int otal_open_set_curves(const double* known, const int* flags, int M, int nthr, double* out, void* stream);" in header
    one = ctypes.c_void_p(16)       # never dereferenced: argument checks come first
    f = lib.otal_open_set_curves
    for k in (0, 1, 4):                                                     # every pointer argument in turn
        args = [one, one, 10, 5, one, None]
        args[k] = None
        assert f(*args) == -1, k                                            # OTAL_E_NULL
    assert f(one, one, -1, 5, one, None) == -2                              # OTAL_E_SHAPE: M < 0
    assert f(one, one, 10, 0, one, None) == -2                              # OTAL_E_SHAPE: nthr < 1
    assert f(one, one, 10, 33, one, None) == -7                             # OTAL_E_UNSUPPORTED: nthr > 32
    assert f(one, one, ops.AP_MAX_CLASS_ROWS + 1, 5, one, None) == -7       # OTAL_E_UNSUPPORTED: more slots than the chunks serve
    assert f(None, one, 10, 33, one, None) == -1                            # the null check comes first
