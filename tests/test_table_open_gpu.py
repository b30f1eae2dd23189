"""GPU: otal_open_set_curves (csrc/oscurve.hip) through table_open.codes_to_curves against the rule on every case of
table_open_cases.py; table_open (torch plumbing -> otal_eval_match -> scatter -> otal_open_set_curves) against open_reference
on tables made by ops.detection_table; and python -m opental_amd.{thumos14,anet}.score_checkpoints --open_metrics on two
randomly initialised checkpoints against the host route (the recipe's test loop -> results_json -> ANETdetection(openset=True)
pre_evaluate -> evaluate('AUC'), evaluate('OSDR')).

Tolerances (table_open.tolerance, derived in the module's docstring): AUROC, AUPR and OSDR within 4 (n + 2) 2^-53 of the rule,
n the foreground's size; FAR@95 bit-equal, NaN for NaN.  Against the host route, which stores float32: within one float32 ulp of
its values, FAR@95 equal after the same cast."""
import json
import os
import sys
import warnings

import numpy as np
import pytest
import torch
import yaml

import table_open_cases as cases

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))

KERNEL_CASES = cases.kernel_cases()


@pytest.fixture(scope="module")
def reference():
    """codes_reference of every kernel case, computed once."""
    from opental_amd.evaluation.table_open import codes_reference
    return {c['name']: codes_reference(c['codes'], c['row'], c['known'], c['cls'], c['gt_cls'], c['ood_threshold'])
            for c in KERNEL_CASES}


def _device_curves(case):
    from opental_amd.evaluation.table_open import codes_to_curves
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return codes_to_curves(up(case['codes']), up(case['row']), up(case['known']), up(case['cls']), up(case['gt_cls']),
                           case['ood_threshold']).cpu().numpy()


def _compare(name, got, want, n):
    from opental_amd.evaluation.table_open import tolerance
    assert got.dtype == np.float64 and got.shape == want.shape
    tol = tolerance(n)
    err = float(np.abs(got[:, [0, 1, 3]] - want[:, [0, 1, 3]]).max())
    print(name, "n", n, "max |d|", err, "tolerance", tol, "FAR@95", got[:, 2].tolist(), want[:, 2].tolist())
    assert tol < 1e-12 and err <= tol
    assert np.array_equal(got[:, 2], want[:, 2], equal_nan=True)         # bit-equal, NaN for NaN


@pytest.mark.parametrize("case", KERNEL_CASES, ids=[c['name'] for c in KERNEL_CASES])
def test_kernel_equals_the_rule(case, reference):
    got = _device_curves(case)
    _compare(case['name'], got, reference[case['name']], case['n'])
    if case['name'] == 'pairs20':
        assert got[0, 2] == 1.0
    if case['name'] == 'n1':
        assert got[0, 3] == 0.5
    if case['name'] == 'only_unknown':
        assert np.isnan(got[0, 2]) and got[0, 0] == 0.0


def test_two_runs_give_the_same_bits():
    for name in ('n513', 'tie_over_chunk_edge', 'nthr32'):
        case = next(c for c in KERNEL_CASES if c['name'] == name)
        a, b = _device_curves(case), _device_curves(case)
        assert a.tobytes() == b.tobytes() and (a > 0).any()


def test_wrapper_checks_its_arguments_and_writes_into_out():
    from opental_amd.common import ops
    known = torch.tensor([[0.25, 0.5, 0.75, 0.0]], dtype=torch.float64, device="cuda")
    flags = torch.tensor([[1, 2, 0, -1]], dtype=torch.int32, device="cuda")
    out = torch.full((1, 4), 7.0, dtype=torch.float64, device="cuda")
    assert ops.open_set_curves(known, flags, out=out) is out
    from opental_amd.evaluation.table_open import curves_reference
    want = curves_reference(np.array([0.25, 0.5, 0.75]), np.arange(3), np.array([False, True, False]),
                            np.array([True, False, False]))
    got = out.cpu().numpy()[0]
    assert np.abs(got[[0, 1, 3]] - np.array(want)[[0, 1, 3]]).max() <= 4 * 5 * 2.0 ** -53 and got[2] == want[2]
    empty = ops.open_set_curves(known[:, :0].contiguous(), flags[:, :0].contiguous())
    assert (empty.cpu().numpy() == 0).all() and tuple(empty.shape) == (1, 4)
    with pytest.raises(RuntimeError, match="float64"):
        ops.open_set_curves(known.float(), flags)
    with pytest.raises(RuntimeError, match="nthr"):
        ops.open_set_curves(known, flags[:, :3].contiguous())
    with pytest.raises(RuntimeError, match="out must be"):
        ops.open_set_curves(known, flags, out=out[:, :3].contiguous())
    many = torch.zeros((33, 4), dtype=torch.float64, device="cuda")
    with pytest.raises(RuntimeError, match="otal_open_set_curves"):
        ops.open_set_curves(many, many.int())                                    # nthr > 32


# ------------------------------------------------------------------------------------------- tables -> the four numbers
V, K, TOP_K, N_GT = 3, 4, 300, 150


def _softnms(seed, ties):
    """Synthetic Soft-NMS output (rows (V, K, top_k, 5), counts (V, K)) and the ground truth of videos 0 and 1 (video 2 has
    none): about half of the rows are jittered copies of a ground truth of their video.  ties: uncertainties on 16 levels."""
    from opental_amd.evaluation.table_ap import GroundTruth
    rs = np.random.RandomState(seed)
    gt_rows = []
    for v in range(V - 1):
        for _ in range(N_GT):
            s = float(rs.uniform(0, 2000))
            gt_rows.append((v, -1 if rs.rand() < 0.4 else int(rs.randint(K)), s, s + float(rs.uniform(2, 20))))
    rows = np.zeros((V, K, TOP_K, 5), dtype=np.float32)
    counts = rs.randint(TOP_K // 2, TOP_K + 1, (V, K)).astype(np.int32)
    for v in range(V):
        mine = [r for r in gt_rows if r[0] == v]
        for c in range(K):
            for i in range(TOP_K):
                if mine and rs.rand() < 0.5:
                    _, gc, gs, ge = mine[rs.randint(len(mine))]
                    s = gs + float(rs.normal(0, 0.15)) * (ge - gs)
                    e = s + (ge - gs) * float(rs.uniform(0.7, 1.3))
                else:
                    s = float(rs.uniform(0, 2000))
                    e = s + float(rs.uniform(2, 20))
                u = float(rs.randint(1, 16)) / 16.0 if ties else float(rs.uniform(0.01, 0.99))
                rows[v, c, i] = (s, e, rs.uniform(0.05, 1.0), u, rs.uniform(0, 1))
    gt = GroundTruth([r[0] for r in gt_rows], [r[1] for r in gt_rows], [r[2:4] for r in gt_rows], K,
                     {"video_%d" % v: v for v in range(V)})
    return rows, counts, gt


def _det_columns(tables):
    parts = [{k: t[k][:int(t['n'])].cpu().numpy() for k in ('video', 'cls', 'seg', 'known')} for t in tables]
    return {k: np.concatenate([p[k] for p in parts]) for k in ('video', 'cls', 'seg', 'known')}


@pytest.mark.parametrize("ties", [False, True])
@pytest.mark.parametrize("ood_threshold", [None, 0.5])
def test_table_open_equals_the_rule(ties, ood_threshold):
    from opental_amd.common import ops
    from opental_amd.evaluation.table_open import KEYS, open_reference, table_open, table_open_counted
    rows, counts, gt = _softnms(3 + int(ties), ties)
    thresholds = [0.3, 0.5, 0.7]
    # one table per video, as a driver's batches give them
    tables = []
    for v in range(V):
        t = ops.detection_table(torch.from_numpy(rows[v:v + 1]).cuda(), torch.from_numpy(counts[v:v + 1]).cuda(),
                                scoring='uncertainty')
        t['video'] += v
        tables.append(t)
    det = _det_columns(tables)
    assert (det['video'] == V - 1).any() and len(det['video']) == int(counts.sum())
    want = open_reference(det, gt.columns(), thresholds, ood_threshold, n_classes=K)
    got, counter = table_open_counted(tables, gt, thresholds, ood_threshold)
    assert counter == 0                                         # not the fallback
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message="table_open")
        again = table_open(tables, gt, thresholds, ood_threshold)
    stack = lambda d: np.stack([d[k] for k in KEYS], 1)
    assert stack(again).tobytes() == stack(got).tobytes()
    # a ground truth is taken once per threshold: no foreground is larger than the M ground-truth rows
    _compare("table_open ties=%s thr=%s" % (ties, ood_threshold), stack(got), stack(want), len(gt.video))
    assert (want['auroc'] > 0).all() and (want['osdr'] > 0).all()   # both kinds matched at every threshold
    if ties:
        assert len(set(det['known'].tolist())) == 15


def test_nonfinite_tiou_falls_back_to_the_rule():
    from opental_amd.common import ops
    from opental_amd.evaluation.table_ap import GroundTruth
    from opental_amd.evaluation.table_open import KEYS, open_reference, table_open, table_open_counted
    rows = np.zeros((1, 1, 2, 5), dtype=np.float32)
    rows[0, 0, 0] = (5.0, 5.0, 0.9, 0.25, 0.5)                  # zero length, on a zero-length ground truth: tIoU 0 / 0
    rows[0, 0, 1] = (10.0, 20.0, 0.8, 0.5, 0.5)
    table = ops.detection_table(torch.from_numpy(rows).cuda(), torch.full((1, 1), 2, dtype=torch.int32, device="cuda"))
    assert int(table['n']) == 2
    gt = GroundTruth([0, 0], [0, -1], [[5.0, 5.0], [10.0, 20.0]], 1, {"video_0": 0})
    assert table_open_counted([table], gt, [0.5])[1] != 0
    with pytest.warns(UserWarning, match="table_open"):
        got = table_open([table], gt, [0.5])
    want = open_reference(_det_columns([table]), gt.columns(), [0.5], n_classes=1)
    for k in KEYS:
        assert got[k].tobytes() == want[k].tobytes()
    assert want['auroc'][0] == 1.0 or want['auroc'][0] == 0.0   # two entries, one of each kind


# --------------------------------------------------------------------------------------------------------------- the drivers
@pytest.fixture()
def _restore_precision():
    """The drivers select the GEMM operand type for the process (OTAL_DTYPE, default bf16): put it back for the other tests."""
    from opental_amd.common import ops
    old = ops.CONV_PRECISION
    yield
    ops.CONV_PRECISION = old


def _save_checkpoints(recipe, config, dev, directory):
    os.makedirs(directory, exist_ok=True)
    for epoch in (1, 2):
        torch.manual_seed(100 + epoch)
        torch.save(recipe.build(config, dev).state_dict(), os.path.join(directory, f"checkpoint-{epoch}.ckpt"))


def _ground_truth_from(results, class_names, subset, skip_last_video):
    """A ground-truth database written from a first pass's detections: per video up to 24 of its detections with distinct
    segments, spread over its list, as annotations -- every other one of a class outside the known list, the rest in turn of
    the detection's own class and of the next known class.  Every known class also gets one annotation far behind the videos' ends (no detection reaches
    it), so that the mAP beside the open-set numbers is defined.  skip_last_video: the last video gets no annotation at all."""
    database = {}
    names = list(results)
    for name in names[:len(names) - 1 if skip_last_video else len(names)]:
        dets, seen, picked = results[name], set(), []
        for d in dets[::max(len(dets) // 24, 1)]:
            seg = tuple(d['segment'])
            if seg not in seen and seg[1] > seg[0]:
                seen.add(seg)
                picked.append(d)
        annotations = []
        for i, d in enumerate(picked[:24]):
            own = class_names.index(d['label'])
            label = "NotInTheList" if i % 2 == 0 else (d['label'] if i % 4 == 1 else class_names[(own + 1) % len(class_names)])
            annotations.append(dict(label=label, segment=list(d['segment'])))
        database[name] = dict(subset=subset, annotations=annotations)
    far = [dict(label=n, segment=[10000.0 + 10.0 * c, 10004.0 + 10.0 * c]) for c, n in enumerate(class_names)]
    database[names[0]]['annotations'] += far
    return database


def _host_open(recipe, config, dev, directory, detect_all, gt_file, known, tious, dataset, subset, version, tmp_path, scoring):
    """{epoch: (dict of the host's float32 arrays, [(known matched, unknown matched) per threshold])} by the host route."""
    from opental_amd.common.detect import results_json
    from opental_amd.evaluation.eval_detection import ANETdetection
    out = {}
    net = recipe.build(config, dev)
    for epoch in (1, 2):
        net.load_state_dict(torch.load(os.path.join(directory, f"checkpoint-{epoch}.ckpt"), map_location='cpu'))
        with torch.no_grad():
            results = detect_all(net)
        pred_file = str(tmp_path / f"pred_{epoch}.json")
        with open(pred_file, "w") as f:
            json.dump(results_json(results, version=version), f)
        det = ANETdetection(ground_truth_filename=gt_file, prediction_filename=pred_file, cls_idx_detection=known, subset=subset,
                            tiou_thresholds=np.asarray(tious), dataset=dataset, openset=True, ood_threshold=None,
                            ood_scoring=scoring, device='cpu')
        det.pre_evaluate()
        auroc, aupr, far = det.evaluate('AUC')
        osdr = det.evaluate('OSDR')
        kinds = [(len(s['known']), len(s['unknown'])) for s in det.eval_data[0]]
        out[epoch] = (dict(AUROC=auroc, AUPR=aupr, FAR95=far, OSDR=osdr), kinds)
    return out


def _check_open(S, argv, map_file, result, want, capsys):
    from opental_amd.common.score_checkpoints import best_epoch
    on_disk = json.load(open(map_file))
    assert on_disk == json.loads(json.dumps(result)) and sorted(on_disk) == ['1', '2', 'best']
    both = False
    for epoch in (1, 2):
        host, kinds = want[epoch]
        entry = on_disk[str(epoch)]
        assert sorted(entry) == ['AUPR', 'AUROC', 'FAR95', 'OSDR', 'average_mAP', 'mAP']
        both = both or any(k > 0 and u > 0 for k, u in kinds)
        for key in ('AUROC', 'AUPR', 'OSDR', 'FAR95'):
            got = np.array([np.nan if v is None else v for v in entry[key]], dtype=np.float64).astype(np.float32)
            with capsys.disabled():
                print("epoch", epoch, key, got.tolist(), "host", host[key].tolist(), "matched (known, unknown)", kinds)
            assert got.shape == host[key].shape and host[key].dtype == np.float32
            if key == 'FAR95':
                assert np.array_equal(got, host[key], equal_nan=True)
            else:
                assert (np.abs(got - host[key]) <= np.spacing(np.abs(host[key]))).all(), key
    assert both                             # at least one threshold has both kinds matched: the comparison is not one of zeros
    assert on_disk['best'] == best_epoch(on_disk, 'average_mAP')
    text_before = open(map_file).read()
    # --select FAR95: nothing is scored again, and the lower mean is best
    capsys.readouterr()
    _, selected = S.main(argv + ['--open_metrics', '--select', 'FAR95'])
    assert capsys.readouterr().out.count("skipped") == 2
    means = {e: float(np.mean([np.nan if v is None else v for v in on_disk[str(e)]['FAR95']])) for e in (1, 2)}
    finite = {e: m for e, m in means.items() if m == m}
    # the lowest mean, the earlier epoch of two equal ones, never a NaN mean
    assert selected['best'] == (min(sorted(finite), key=lambda e: finite[e]) if finite else None)
    assert open(map_file).read() == text_before                 # nothing was scored: the file was not written
    # without the new flags both epochs hold what is asked for: the file keeps its content
    mtime = os.path.getmtime(map_file)
    _, plain = S.main(argv)
    assert capsys.readouterr().out.count("skipped") == 2 and plain['best'] == on_disk['best']
    assert open(map_file).read() == text_before and os.path.getmtime(map_file) == mtime


def test_thumos14_driver_scores_the_open_set_numbers(tmp_path, capsys, monkeypatch, _restore_precision):
    from make_synthetic_thumos import CLASSES, make
    from opental_amd.common import config as C
    from opental_amd.common.driver import device_setup
    from opental_amd.common.thumos_dataset import get_class_index_map, get_video_info
    from opental_amd.thumos14 import score_checkpoints as S, test as T
    data = tmp_path / "data"
    yaml_path = make(str(data), videos=1, frames=100, size=96, test_videos=0)
    rs = np.random.RandomState(5)
    names = [f"video_test_{v:07d}" for v in range(4)]
    rows = ["video,fps,sample_fps,count,sample_count"]
    for name in names:
        np.save(str(data / "test_npy" / (name + ".npy")), rs.randint(0, 256, (300, 96, 96, 3)).astype(np.uint8))
        rows.append(f"{name},30.0,10.0,900,300")
    (data / "test_info.csv").write_text("\n".join(rows) + "\n")
    gt_file, known, run_dir = str(data / "gt_open.json"), str(data / "classes.txt"), str(tmp_path / "run")
    argv = [yaml_path, '--open_set', '--split', '0', '--checkpoint_path', run_dir, '--gt', gt_file, '--known', known]
    config = C.get_config(argv[:6])
    dev = torch.device("cuda", 0)
    _save_checkpoints(S.RECIPE, config, dev, run_dir)
    te, ds = config['testing'], config['dataset']['testing']
    infos = get_video_info(ds['video_info_path'])
    assert list(infos) == names
    detect_all = lambda net: T.test(net, infos, ds['video_data_path'], get_class_index_map(known)[1], ds['clip_length'],
                                    ds['clip_stride'], ds['crop_size'], te['conf_thresh'], te['top_k'], te['nms_sigma'], device=dev)
    # the ground truth comes from a first pass's detections (the first checkpoint's), half of them of an unknown class
    device_setup()                              # the operand type the driver will select: the passes see the same detections
    net = S.RECIPE.build(config, dev)
    net.load_state_dict(torch.load(os.path.join(run_dir, "checkpoint-1.ckpt"), map_location='cpu'))
    with torch.no_grad():
        first = detect_all(net)
    assert sum(len(v) for v in first.values()) > 0
    json.dump(dict(database=_ground_truth_from(first, [n for _, n in CLASSES], "test", skip_last_video=True)), open(gt_file, "w"))
    map_file, result = S.main(argv + ['--open_metrics'])
    assert map_file == os.path.join(run_dir, "checkpoint_map.json")
    want = _host_open(S.RECIPE, config, dev, run_dir, detect_all, gt_file, known, S.RECIPE.tious, 'thumos14', ['test'], "THUMOS14",
                      tmp_path, te['ood_scoring'])
    monkeypatch.setattr(S.RECIPE, "build", lambda *a: pytest.fail("a skipped epoch must not build the network"))
    _check_open(S, argv, map_file, result, want, capsys)


def test_anet_driver_scores_the_open_set_numbers(tmp_path, capsys, monkeypatch, _restore_precision):
    from make_synthetic_anet import make
    from opental_amd.anet import score_checkpoints as S, test as AT
    from opental_amd.common import config as C
    from opental_amd.common.driver import device_setup
    root = tmp_path / "anet"
    yaml_path = make(str(root), videos=2, size=96)
    cfg = yaml.load(open(yaml_path).read(), Loader=yaml.FullLoader)
    cfg['testing']['conf_thresh'] = 0.0005      # a random network spreads its score over 150 classes: below the recipe's 0.01
    with open(yaml_path, "w") as f:
        yaml.dump(cfg, f)
    rs = np.random.RandomState(9)
    class_names = [f"class_{i}" for i in range(150)]
    info = {}
    for v in range(2):
        name = f"v_synth{v:05d}"
        np.save(str(root / "train_val_npy" / (name + ".npy")), rs.randint(0, 256, (768, 96, 96, 3)).astype(np.uint8))
        info[name] = dict(subset="validation", fps=10.0, frame_num=768, duration=76.8, annotations=[])
    json.dump(info, open(root / "video_info.json", "w"))
    gt_file, known, run_dir = str(root / "gt_open.json"), str(root / "action_known.txt"), str(tmp_path / "run")
    argv = [yaml_path, '--open_set', '--split', '0', '--checkpoint_path', run_dir, '--gt', gt_file, '--known', known]
    config = C.get_config(argv[:6])
    dev = torch.device("cuda", 0)
    _save_checkpoints(S.RECIPE, config, dev, run_dir)
    te, t = config['testing'], config['dataset']['testing']
    assert list(AT.get_class_names(known).values()) == class_names
    detect_all = lambda net: AT.testing(net, list(info), info, t['video_mp4_path'], AT.get_class_names(known), t['clip_length'],
                                        t['crop_size'], te['conf_thresh'], te['top_k'], te['nms_sigma'], device=dev)
    device_setup()                              # the operand type the driver will select: the passes see the same detections
    net = S.RECIPE.build(config, dev)
    net.load_state_dict(torch.load(os.path.join(run_dir, "checkpoint-1.ckpt"), map_location='cpu'))
    with torch.no_grad():
        first = detect_all(net)
    assert sorted(first) == [n[2:] for n in info] and sum(len(v) for v in first.values()) > 0
    json.dump(dict(database=_ground_truth_from(first, class_names, "validation", skip_last_video=False)), open(gt_file, "w"))
    map_file, result = S.main(argv + ['--open_metrics'])
    want = _host_open(S.RECIPE, config, dev, run_dir, detect_all, gt_file, known, S.RECIPE.tious, 'anet', ['validation'],
                      "ActivityNet-v1.3", tmp_path, te['ood_scoring'])
    monkeypatch.setattr(S.RECIPE, "build", lambda *a: pytest.fail("a skipped epoch must not build the network"))
    _check_open(S, argv, map_file, result, want, capsys)
