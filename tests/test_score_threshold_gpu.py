"""GPU: python -m opental_amd.{thumos14,anet}.score_checkpoints --open_metrics --threshold_from_train --wi on two randomly
initialised checkpoints and a few synthetic videos that the training and the test list share.

  * every epoch's "ood_threshold" equals, as a float, what the recipe's own thresholding(...) returns for the same network and
    videos: both sort the same fp64 known-ness values;
  * its "WI" and its four curves equal the host route -- the recipe's test loop -> results_json -> ANETdetection(openset=True,
    ood_threshold=that threshold, device='cpu') -- to their tolerances: the curves within one float32 ulp of the host's float32
    (FAR@95 equal after the cast, as in test_table_open_gpu.py), the per-tIoU mean WI within table_wi.tolerance(m), m = the
    unknown ground truths + 1 (the bound holds per class, so for their mean);
  * a second run skips every epoch, a run under another --threshold_videos scores again.

The ground truth is written from a first pass's detections (half of them of a class outside the list), so the matching has
something to find, and the test asserts that the threshold relabels at least one scored detection and leaves at least one.  A
plainly random network cannot pass that: its known-ness lies on one side of 0.5, so `1 - known < threshold` holds for all of
its detections or for none.  _save_checkpoints therefore shifts the classification biases of each checkpoint so that the median
known-ness is 0.5 (--ood_scoring uncertainty)."""
import json
import os
import sys

import numpy as np
import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
FLAGS = ['--open_metrics', '--threshold_from_train', '--wi']


def _save_checkpoints(recipe, config, dev, directory):
    """Two randomly initialised checkpoints whose classification biases are shifted so that the threshold relabels some
    detections and not all.  The protocol relabels a detection where 1 - known < threshold, the threshold being the 5 %
    quantile of known: with a random network's known-ness all above 0.5 (uncertainty = K / (K + the summed exp evidence), the
    evidence sum a little above K) that is every detection, and with all of it below 0.5 none.  Adding log(u / (1 - u)), u the
    median uncertainty over the videos, to the biases of conf_head and prop_conf_head scales every evidence sum by that factor
    and puts the median known-ness on 0.5: the 5 % quantile q lies below it and the detections above 1 - q are relabelled."""
    os.makedirs(directory, exist_ok=True)
    _, state = recipe.train_videos(config)
    batches = recipe.batches(config, state)
    for epoch in (1, 2):
        torch.manual_seed(100 + epoch)
        net = recipe.build(config, dev)
        with torch.no_grad():
            known = torch.cat([t['known'][:int(t['n'])] for t in (recipe.train_table(net, config, state, part, dev, scoring='uncertainty')
                                                                 for part in batches)])
            u = 1.0 - float(known.median())
            shifted = 0
            for key, value in net.state_dict().items():
                if 'conf_head' in key and key.endswith('bias'):
                    value += float(np.log(u / (1.0 - u)))
                    shifted += 1
        assert 0.0 < u < 1.0 and shifted == 2, (u, shifted)
        torch.save(net.state_dict(), os.path.join(directory, f"checkpoint-{epoch}.ckpt"))


def _ground_truth_from(results, class_names, subset, skip_last_video):
    """A ground-truth database written from a first pass's detections, as test_table_open_gpu.py writes it: per video up to 24
    of its detections with distinct segments as annotations -- every other one of a class outside the known list, the rest in
    turn of the detection's own class and of the next known class -- and one annotation per known class far behind the
    videos' ends, so that the mAP is defined.  skip_last_video: the last video gets no annotation at all."""
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


@pytest.fixture(autouse=True)
def _restore_precision():
    """The drivers select the GEMM operand type for the process (OTAL_DTYPE, default bf16): put it back for the other tests."""
    from opental_amd.common import ops
    old = ops.CONV_PRECISION
    yield
    ops.CONV_PRECISION = old


def _host_route(recipe, config, dev, directory, detect_all, threshold_of, gt_file, known, tious, dataset, subset, version, tmp_path,
                scoring):
    """{epoch: dict(threshold, the host's four float32 arrays, WI fp64 (nthr, K), relabelled / kept counts, m)}."""
    from opental_amd.common.detect import results_json
    from opental_amd.evaluation.eval_detection import ANETdetection
    out = {}
    net = recipe.build(config, dev)
    for epoch in (1, 2):
        net.load_state_dict(torch.load(os.path.join(directory, f"checkpoint-{epoch}.ckpt"), map_location='cpu'))
        with torch.no_grad():
            thr = threshold_of(net, str(tmp_path / f"threshold_{epoch}.json"))
            results = detect_all(net)
        pred_file = str(tmp_path / f"pred_{epoch}.json")
        with open(pred_file, "w") as f:
            json.dump(results_json(results, version=version), f)
        det = ANETdetection(ground_truth_filename=gt_file, prediction_filename=pred_file, cls_idx_detection=known, subset=subset,
                            tiou_thresholds=np.asarray(tious), dataset=dataset, openset=True, ood_threshold=thr,
                            ood_scoring=scoring, device='cpu')
        det.pre_evaluate()
        auroc, aupr, far = det.evaluate('AUC')
        osdr = det.evaluate('OSDR')
        wi = det.evaluate('WI')[2]
        label = det.prediction['label']
        out[epoch] = dict(threshold=thr, AUROC=auroc, AUPR=aupr, FAR95=far, OSDR=osdr, WI=wi, relabelled=int((label == 0).sum()),
                          kept=int((label > 0).sum()), m=int((det.ground_truth['label'] == 0).sum()) + 1,
                          tp_u2u=float(det.stats['tp_u2u'].sum()))
    return out


def _check(S, argv, map_file, result, want, capsys, nthr):
    from opental_amd.evaluation.table_wi import tolerance
    on_disk = json.load(open(map_file))
    assert on_disk == json.loads(json.dumps(result)) and sorted(on_disk) == ['1', '2', 'best']
    for epoch in (1, 2):
        host, entry = want[epoch], on_disk[str(epoch)]
        assert sorted(entry) == ['AUPR', 'AUROC', 'FAR95', 'OSDR', 'WI', 'average_mAP', 'mAP', 'ood_threshold', 'ood_threshold_from']
        assert entry['ood_threshold_from'] == 'train'
        with capsys.disabled():
            print("epoch", epoch, "threshold", entry['ood_threshold'], "host", host['threshold'], "relabelled", host['relabelled'],
                  "kept", host['kept'], "tp_u2u", host['tp_u2u'])
        assert isinstance(entry['ood_threshold'], float) and entry['ood_threshold'] == host['threshold']
        # the comparison shows something: the threshold relabels some scored detections and not all
        assert host['relabelled'] >= 1 and host['kept'] >= 1
        for key in ('AUROC', 'AUPR', 'OSDR', 'FAR95'):
            got = np.array([np.nan if v is None else v for v in entry[key]], dtype=np.float64).astype(np.float32)
            assert got.shape == host[key].shape == (nthr,) and host[key].dtype == np.float32
            if key == 'FAR95':
                assert np.array_equal(got, host[key], equal_nan=True)
            else:
                assert (np.abs(got - host[key]) <= np.spacing(np.abs(host[key]))).all(), key
        got, mean = np.array(entry['WI'], dtype=np.float64), host['WI'].mean(axis=1)
        tol = tolerance(host['m'])
        with capsys.disabled():
            print("epoch", epoch, "WI", got.tolist(), "host", mean.tolist(), "max |d|", float(np.abs(got - mean).max()), "tolerance", tol)
        assert got.shape == mean.shape == (nthr,) and tol < 1e-12 and (mean > 0).any()
        assert (np.abs(got - mean) <= tol).all()
    text_before = open(map_file).read()
    # a second run finds both epochs in the file, with their own thresholds, and scores nothing
    capsys.readouterr()
    _, again = S.main(argv + FLAGS)
    assert capsys.readouterr().out.count("skipped") == 2 and again == result and open(map_file).read() == text_before
    # --select WI: nothing is scored either, and the lowest mean is best
    _, selected = S.main(argv + FLAGS + ['--select', 'WI'])
    assert capsys.readouterr().out.count("skipped") == 2
    means = {e: float(np.mean(on_disk[str(e)]['WI'])) for e in (1, 2)}
    assert selected['best'] == (1 if means[1] <= means[2] else 2)


def _check_another_cap(S, argv, map_file, result, capsys):
    """Another --threshold_videos: the entry was made without a cap, so the epoch is scored again and records the cap."""
    capsys.readouterr()
    _, capped = S.main(argv + FLAGS + ['--threshold_videos', '1', '--epochs', '1'])
    text = capsys.readouterr().out
    assert "skipped" not in text and " WI " in text and " thr " in text
    entry = capped['1']
    assert entry['threshold_videos'] == 1 and entry['ood_threshold_from'] == 'train' and isinstance(entry['ood_threshold'], float)
    assert capped['2'] == result['2'] and json.load(open(map_file))['1'] == entry
    _, held = S.main(argv + FLAGS + ['--threshold_videos', '1', '--epochs', '1'])
    assert capsys.readouterr().out.count("skipped") == 1 and held['1'] == entry


def test_thumos14_epochs_are_scored_at_their_own_threshold(tmp_path, capsys, monkeypatch):
    from make_synthetic_thumos import CLASSES, make
    from opental_amd.common import config as C
    from opental_amd.common.driver import device_setup
    from opental_amd.common.thumos_dataset import get_class_index_map, get_video_info
    from opental_amd.thumos14 import score_checkpoints as S, test as T, threshold as TH
    data = tmp_path / "data"
    yaml_path = make(str(data), videos=1, frames=100, size=96, test_videos=0)
    rs = np.random.RandomState(5)
    names = [f"video_test_{v:07d}" for v in range(3)]
    rows = ["video,fps,sample_fps,count,sample_count"]
    for name in names:                                   # the training and the test list share their videos
        clip = rs.randint(0, 256, (300, 96, 96, 3)).astype(np.uint8)
        for part in ("test_npy", "train_npy"):
            np.save(str(data / part / (name + ".npy")), clip)
        rows.append(f"{name},30.0,10.0,900,300")
    for fn in ("test_info.csv", "train_info.csv"):
        (data / fn).write_text("\n".join(rows) + "\n")
    gt_file, known, run_dir = str(data / "gt_open.json"), str(data / "classes.txt"), str(tmp_path / "run")
    argv = [yaml_path, '--open_set', '--split', '0', '--ood_scoring', 'uncertainty', '--checkpoint_path', run_dir, '--gt', gt_file,
            '--known', known]
    config = C.get_config(argv[:8])
    dev = torch.device("cuda", 0)
    device_setup()                              # the operand type the driver will select: the passes see the same detections
    _save_checkpoints(S.RECIPE, config, dev, run_dir)
    te, ds, tr = config['testing'], config['dataset']['testing'], config['dataset']['training']
    infos, train_infos = get_video_info(ds['video_info_path']), get_video_info(tr['video_info_path'])
    assert list(infos) == names == list(train_infos)
    idx_to_class = get_class_index_map(known)[1]
    detect_all = lambda net: T.test(net, infos, ds['video_data_path'], idx_to_class, ds['clip_length'], ds['clip_stride'],
                                    ds['crop_size'], te['conf_thresh'], te['top_k'], te['nms_sigma'], device=dev)
    threshold_of = lambda net, path: TH.thresholding(net, train_infos, tr['video_data_path'], path, idx_to_class, te['ood_scoring'],
                                                     ds['clip_length'], ds['clip_stride'], ds['crop_size'], te['conf_thresh'],
                                                     te['top_k'], te['nms_sigma'], device=dev)
    net = S.RECIPE.build(config, dev)
    net.load_state_dict(torch.load(os.path.join(run_dir, "checkpoint-1.ckpt"), map_location='cpu'))
    with torch.no_grad():
        first = detect_all(net)
    assert sum(len(v) for v in first.values()) > 0
    json.dump(dict(database=_ground_truth_from(first, [n for _, n in CLASSES], "test", skip_last_video=True)), open(gt_file, "w"))
    map_file, result = S.main(argv + FLAGS)
    text = capsys.readouterr().out
    assert text.count(" WI ") == 2 and text.count(" thr ") == 2
    want = _host_route(S.RECIPE, config, dev, run_dir, detect_all, threshold_of, gt_file, known, S.RECIPE.tious, 'thumos14', ['test'],
                       "THUMOS14", tmp_path, te['ood_scoring'])
    build = S.RECIPE.build
    monkeypatch.setattr(S.RECIPE, "build", lambda *a: pytest.fail("a skipped epoch must not build the network"))
    _check(S, argv, map_file, result, want, capsys, 5)
    monkeypatch.setattr(S.RECIPE, "build", build)
    _check_another_cap(S, argv, map_file, result, capsys)


def test_anet_epochs_are_scored_at_their_own_threshold(tmp_path, capsys, monkeypatch):
    from make_synthetic_anet import make
    from opental_amd.anet import score_checkpoints as S, test as AT, threshold as TH
    from opental_amd.common import config as C
    from opental_amd.common.driver import device_setup
    root = tmp_path / "anet"
    yaml_path = make(str(root), videos=2, size=96)
    cfg = yaml.load(open(yaml_path).read(), Loader=yaml.FullLoader)
    cfg['testing']['conf_thresh'] = 0.0005      # a random network spreads its score over 150 classes: below the recipe's 0.01
    cfg['dataset']['training']['video_info_path'] = str(root / "video_info_train.json")
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
    # the same videos as the training split of a second info file
    json.dump({n: dict(v, subset="training") for n, v in info.items()}, open(root / "video_info_train.json", "w"))
    gt_file, known, run_dir = str(root / "gt_open.json"), str(root / "action_known.txt"), str(tmp_path / "run")
    tious = ['0.5', '0.75', '0.95']             # three of the recipe's ten: the host's WI holds four (nthr, 150, N) fp64 arrays
    argv = [yaml_path, '--open_set', '--split', '0', '--ood_scoring', 'uncertainty', '--checkpoint_path', run_dir, '--gt', gt_file,
            '--known', known, '--tious'] + tious
    config = C.get_config(argv[:8])
    dev = torch.device("cuda", 0)
    device_setup()                              # the operand type the driver will select: the passes see the same detections
    _save_checkpoints(S.RECIPE, config, dev, run_dir)
    te, t, tr = config['testing'], config['dataset']['testing'], config['dataset']['training']
    idx_to_class = AT.get_class_names(known)
    detect_all = lambda net: AT.testing(net, list(info), info, t['video_mp4_path'], idx_to_class, t['clip_length'], t['crop_size'],
                                        te['conf_thresh'], te['top_k'], te['nms_sigma'], device=dev)
    train_list, train_infos = TH.select_videos(tr['video_info_path'], tr['video_mp4_path'])
    assert train_list == list(info)
    threshold_of = lambda net, path: TH.thresholding(net, train_list, train_infos, tr['video_mp4_path'], path, idx_to_class,
                                                     te['ood_scoring'], t['clip_length'], t['crop_size'], te['conf_thresh'],
                                                     te['top_k'], te['nms_sigma'], device=dev)
    net = S.RECIPE.build(config, dev)
    net.load_state_dict(torch.load(os.path.join(run_dir, "checkpoint-1.ckpt"), map_location='cpu'))
    with torch.no_grad():
        first = detect_all(net)
    assert sorted(first) == [n[2:] for n in info] and sum(len(v) for v in first.values()) > 0
    json.dump(dict(database=_ground_truth_from(first, class_names, "validation", skip_last_video=False)), open(gt_file, "w"))
    map_file, result = S.main(argv + FLAGS)
    text = capsys.readouterr().out
    assert text.count(" WI ") == 2 and text.count(" thr ") == 2
    want = _host_route(S.RECIPE, config, dev, run_dir, detect_all, threshold_of, gt_file, known, [float(x) for x in tious], 'anet',
                       ['validation'], "ActivityNet-v1.3", tmp_path, te['ood_scoring'])
    build = S.RECIPE.build
    monkeypatch.setattr(S.RECIPE, "build", lambda *a: pytest.fail("a skipped epoch must not build the network"))
    _check(S, argv, map_file, result, want, capsys, 3)
    monkeypatch.setattr(S.RECIPE, "build", build)
    _check_another_cap(S, argv, map_file, result, capsys)
