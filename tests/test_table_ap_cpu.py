"""CPU: the rule of opental_amd/evaluation/table_ap.py (ap_reference) against the host evaluator
(ANETdetection(device='cpu').evaluate('AP')) through the real file layout, in both protocols and on the golden fixture; its tie
rule against a hand-computed value; the GroundTruth loader against ANETdetection._import_ground_truth; and
otal_average_precision's argument codes.

Tolerance (table_ap.tolerance, derived in the module's docstring): both sides hold the same integer counts and the same fp64
quotients and differ in the order of adding at most npos terms: |dAP| <= 4 npos 2^-53 with the case's own npos."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import table_ap_cases as cases
from eval_match_cases import TIOUS as FIXTURE_TIOUS, detector, fixture_paths

BASE = cases.base_cases()
OPEN = [cases.with_unknown(c) for c in BASE]
REFERENCE_ONLY = cases.reference_only_cases()


def _ids(cs):
    return [c['name'] for c in cs]


def _host_ap(case, directory, openset):
    from opental_amd.evaluation.eval_detection import ANETdetection
    gt_file, pred_file, cls_file = cases.write_files(case, directory)
    det = ANETdetection(ground_truth_filename=gt_file, prediction_filename=pred_file, cls_idx_detection=cls_file,
                        subset=['test'], tiou_thresholds=np.array(case['thresholds']), dataset='thumos14', openset=openset,
                        ood_threshold=None, device='cpu')
    return det.evaluate('AP')[2]


def _check(case, want):
    from opental_amd.evaluation.table_ap import ap_reference, tolerance
    got = ap_reference(case['det'], case['gt'], case['thresholds'], case['n_classes'])
    assert got.dtype == np.float64 and got.shape == (len(case['thresholds']), case['n_classes'])
    tol = tolerance(cases.npos_max(case))
    err = float(np.abs(got - want).max())
    print(case['name'], "npos", cases.npos_max(case), "max |dAP|", err, "tolerance", tol)
    assert tol < 1e-12 and err <= tol
    return got


def test_case_list_covers_what_it_says():
    by_name = {c['name']: c for c in BASE}
    det = by_name['class_sizes']['det']
    kept = np.isin(det['video'], by_name['class_sizes']['gt']['video'])         # without the video that has no ground truth
    assert not kept.all()
    assert tuple(np.bincount(det['cls'][kept])) == cases.CLASS_SIZES == (1, cases.TILE - 1, cases.TILE, cases.TILE + 1,
                                                                        2 * cases.TILE + 3)
    assert [len(by_name[n]['thresholds']) for n in ('nthr1', 'nthr10', 'nthr32')] == [1, 10, 32]
    assert by_name['150x3']['n_classes'] == 150 and by_name['15x6']['n_classes'] == 15
    for c in BASE:
        assert c['host'] and (c['gt']['cls'] >= 0).all()
        # distinct scores inside every class: the host's argsort()[::-1] is determined
        pairs = set(zip(c['det']['cls'].tolist(), c['det']['score'].tolist()))
        assert len(pairs) == len(c['det']['cls']), c['name']
    for c in OPEN:
        assert (c['gt']['cls'] == -1).sum() == 1
        pairs = set(zip(c['det']['cls'].tolist(), c['det']['score'].tolist()))
        assert len(pairs) == len(c['det']['cls']), c['name']
    assert not any(c['host'] for c in REFERENCE_ONLY)


def test_tile_constant_is_the_header_s():
    from opental_amd.common import ops
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "opental_hip.h")).read()
    assert int(re.search(r"#define OTAL_AP_TILE (\d+)", header).group(1)) == ops.AP_TILE
    assert "#define OTAL_AP_MAX_CLASS_ROWS (2147483647 - OTAL_AP_TILE)" in header
    assert ops.AP_MAX_CLASS_ROWS == 2147483647 - ops.AP_TILE


@pytest.mark.parametrize("case", BASE, ids=_ids(BASE))
def test_reference_equals_the_host_evaluator_closed_set(case, tmp_path):
    ap = _check(case, _host_ap(case, tmp_path, openset=False))
    if case['name'] == 'empty_fp_tp':
        assert (ap[:, [1, 2, 4]] == 0).all() and (ap[:, 3] == 1.0).all() and (ap[:, [0, 5]] > 0).all()
        assert (ap[:, [0, 5]] < 1).all()


@pytest.mark.parametrize("case", OPEN, ids=_ids(OPEN))
def test_reference_equals_the_host_evaluator_open_set(case, tmp_path):
    want = _host_ap(case, tmp_path, openset=True)           # one column per known class, '__unknown__' last
    assert want.shape[1] == case['n_classes'] + 1 and (want[:, -1] == 0).all()
    _check(case, want[:, :case['n_classes']])


def test_detections_of_the_unknown_only_video_are_false_positives():
    from opental_amd.evaluation.table_ap import ap_reference
    det = dict(video=np.array([0, 1], dtype=np.int32), cls=np.zeros(2, dtype=np.int32),
               seg=np.array([[0.0, 10.0], [0.0, 10.0]]), score=np.array([0.4, 0.9], dtype=np.float32))
    gt = dict(video=np.array([0, 1], dtype=np.int32), cls=np.array([0, -1], dtype=np.int32),
              seg=np.array([[0.0, 10.0], [0.0, 10.0]]))
    # video 1's only ground truth is of an unknown class: its detection is kept, ranks first and is a false positive
    assert ap_reference(det, gt, [0.5], 1).tolist() == [[0.5]]
    # without that row video 1 has no ground truth at all and its detection is dropped
    assert ap_reference(det, {k: v[:1] for k, v in gt.items()}, [0.5], 1).tolist() == [[1.0]]


def _fixture_columns(paths, gt_file):
    from opental_amd.evaluation.table_ap import GroundTruth
    gt = GroundTruth.load(paths[gt_file], paths["eval_classes.txt"], subset=['test'], dataset='thumos14')
    class_to_idx = {}
    for i, line in enumerate(open(paths["eval_classes.txt"]).read().splitlines()):
        class_to_idx[line.split()[1]] = i
    rows = [(gt.video_index.get(vid, len(gt.video_index)), class_to_idx[r['label']], r['segment'], r['score'])
            for vid, dets in json.load(open(paths["eval_pred.json"]))['results'].items() for r in dets
            if r['label'] in class_to_idx]
    det = dict(video=np.array([r[0] for r in rows], dtype=np.int32), cls=np.array([r[1] for r in rows], dtype=np.int32),
               seg=np.array([r[2] for r in rows], dtype=np.float64), score=np.array([r[3] for r in rows], dtype=np.float64))
    return det, gt


@pytest.mark.parametrize("gt_file,openset", [("eval_gt_closed.json", False), ("eval_gt_open.json", True)])
def test_reference_on_the_golden_fixture(golden_dir, gt_file, openset):
    from opental_amd.evaluation.table_ap import ap_reference, tolerance
    paths = fixture_paths(golden_dir)
    det, gt = _fixture_columns(paths, gt_file)
    host = detector(paths, gt_file, openset=openset, device='cpu')
    want = host.evaluate('AP')[2][:, :gt.n_classes]
    got = ap_reference(det, gt.columns(), FIXTURE_TIOUS, gt.n_classes)
    tol = tolerance(int(gt.gt_count.max()))
    print("max |dAP|", float(np.abs(got - want).max()), "tolerance", tol)
    assert np.abs(got - want).max() <= tol
    if not openset:
        pinned = np.array(json.load(open(paths["eval_expected.json"]))["closed"]["ap"])
        assert np.abs(got - pinned).max() < 1e-12


def test_equal_scores_go_by_table_row():
    from opental_amd.evaluation.table_ap import ap_reference, tolerance
    case = cases.tie_case()
    ap = ap_reference(case['det'], case['gt'], case['thresholds'], 1)
    assert abs(ap[0, 0] - cases.TIE_AP) <= tolerance(2)
    # the rows of the tie the other way round: true positives first
    flipped = {k: v[[1, 2, 0, 3]] for k, v in case['det'].items()}
    assert abs(ap_reference(flipped, case['gt'], case['thresholds'], 1)[0, 0] - 2.0 / 3.0) <= tolerance(2)


def test_shared_tiou_takes_the_lower_ground_truth_row():
    from opental_amd.evaluation.table_ap import ap_reference
    case = cases.shared_tiou_case(chain=True)
    ap = ap_reference(case['det'], case['gt'], case['thresholds'], 1)
    # at 0.5 and 0.6: [10, 20] takes row 0 ([10, 25]), [50, 61] matches, [70, 80] misses, [6, 20] takes the free [5, 20]:
    # precision 1, 1, 2/3, 3/4 and recall 1/3, 2/3, 2/3, 1 -> 1/3 + 1/3 + (1/3) (3/4)
    assert np.allclose(ap[:2, 0], 2.0 / 3.0 + 0.25, rtol=0, atol=1e-15)
    # (had [10, 20] taken row 1, [6, 20] would find only [10, 25], tIoU 10 / 19: a miss at 0.6 and AP 2/3)
    # at 0.9 [50, 61] (10 / 11) and [6, 20] (14 / 15) match: precision 0, 1/2, 1/3, 2/4 -> envelope 1/2 -> 2 (1/3) (1/2)
    assert np.allclose(ap[2, 0], 1.0 / 3.0, rtol=0, atol=1e-15)


def test_class_without_ground_truth_raises_keyerror():
    from opental_amd.evaluation.table_ap import ap_reference
    case = BASE[0]
    with pytest.raises(KeyError) as e:
        ap_reference(case['det'], case['gt'], case['thresholds'], 3)
    assert e.value.args == (2,)             # classes are 1-based in the host path's message


@pytest.mark.parametrize("openset", [False, True])
def test_ground_truth_loader_equals_import_ground_truth(tmp_path, openset):
    from opental_amd.evaluation.eval_detection import ANETdetection
    from opental_amd.evaluation.table_ap import GroundTruth
    case = OPEN[1] if openset else BASE[1]
    gt_file, pred_file, cls_file = cases.write_files(case, tmp_path)
    database = json.load(open(gt_file))
    database['database']['other_subset'] = dict(subset='validation', annotations=[dict(label='Class000', segment=[0.0, 1.0])])
    json.dump(database, open(gt_file, 'w'))
    host = ANETdetection(ground_truth_filename=gt_file, prediction_filename=pred_file, cls_idx_detection=cls_file, subset=['test'],
                         tiou_thresholds=np.array(cases.TIOUS), dataset='thumos14', openset=openset)
    gt = GroundTruth.load(gt_file, cls_file, subset=['test'], dataset='thumos14')
    want = host.ground_truth
    assert gt.n_classes == case['n_classes'] and len(gt.video) == len(want['label']) == len(case['gt']['cls'])
    assert np.array_equal(gt.cls.astype(np.int64) + 1, want['label'])       # 0 ('__unknown__') <-> -1
    assert np.array_equal(gt.seg[:, 0], want['t-start']) and np.array_equal(gt.seg[:, 1], want['t-end'])
    names = {i: n for n, i in gt.video_index.items()}
    assert [names[v] for v in gt.video.tolist()] == want['video-id'].tolist() and 'other_subset' not in gt.video_index
    assert np.array_equal(gt.gt_count, np.bincount(want['label'], minlength=gt.n_classes + 1)[1:])
    # a driver's own video list is numbered first, in its order, whether the videos have ground truth or not
    mine = ['no_ground_truth', cases.video_name(3), cases.video_name(0)]
    gt2 = GroundTruth.load(gt_file, cls_file, subset=['test'], dataset='thumos14', videos=mine)
    assert [gt2.video_index[n] for n in mine] == [0, 1, 2] and gt2.nvid == gt.nvid + 1
    assert np.array_equal(gt2.cls, gt.cls) and np.array_equal(gt2.seg, gt.seg)
    # ActivityNet's class file: the whole line is the name
    anet_cls = tmp_path / "anet_classes.txt"
    anet_cls.write_text("".join("Class%03d\n" % c for c in range(case['n_classes'])))
    gt3 = GroundTruth.load(gt_file, str(anet_cls), subset=['test'], dataset='anet')
    assert np.array_equal(gt3.cls, gt.cls)


def test_average_precision_argument_errors_do_not_launch():
    from opental_amd.common import ops
    from opental_amd.csrc import build
    if not os.path.exists(build.LIB):
        build.build(verbose=False)
    from opental_amd._lib import declare
    lib = declare(ctypes.CDLL(build.LIB))
    one = ctypes.c_void_p(16)       # never dereferenced: argument checks come first
    f = lib.otal_average_precision
    for k in (0, 1, 2, 3, 7):                                               # every pointer argument in turn
        args = [one, one, one, one, 10, 2, 5, one, None]
        args[k] = None
        assert f(*args) == -1, k                                            # OTAL_E_NULL
    assert f(one, one, one, one, -1, 2, 5, one, None) == -2                 # OTAL_E_SHAPE: N < 0
    assert f(one, one, one, one, 10, 0, 5, one, None) == -2                 # OTAL_E_SHAPE: K < 1
    assert f(one, one, one, one, 10, 2, 0, one, None) == -2                 # OTAL_E_SHAPE: nthr < 1
    assert f(one, one, one, one, 10, 2, 33, one, None) == -7                # OTAL_E_UNSUPPORTED: nthr > 32
    # OTAL_E_UNSUPPORTED: a class can hold N rows, more than the chunk bookkeeping serves
    assert f(one, one, one, one, ops.AP_MAX_CLASS_ROWS + 1, 2, 5, one, None) == -7
    assert f(None, one, one, one, 10, 2, 33, one, None) == -1               # the null check comes first
