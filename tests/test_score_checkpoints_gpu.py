"""GPU: python -m opental_amd.{thumos14,anet}.score_checkpoints on two randomly initialised checkpoints and a few synthetic
videos: checkpoint_map.json against the host route of the parent tree on the same checkpoints -- the recipe's test loop ->
results_json -> ANETdetection(device='cpu').evaluate('AP') -- and the skipping of epochs already scored.

Tolerance (table_ap.tolerance): |dAP| <= 4 npos 2^-53 per class with the ground truth's largest npos; mAP is the mean of the
per-class values.  The ground truth is dense (every class tiles half a minute of two videos) so that detections of a random
network match some of it and the comparison is not one of zeros."""
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


@pytest.fixture(autouse=True)
def _restore_precision():
    """The drivers select the GEMM operand type for the process (OTAL_DTYPE, default bf16): put it back for the other tests."""
    from opental_amd.common import ops
    old = ops.CONV_PRECISION
    yield
    ops.CONV_PRECISION = old


def _annotations(class_names, v, nvideos, span):
    """Every class tiles [0, span) of half of the videos with six segments, shifted per class; one annotation per video is of
    a class outside the list."""
    out = []
    for c, name in enumerate(class_names):
        if (c + v) % 2 and nvideos > 1:
            continue
        step = span / 6.0
        shift = (c % 5) * step / 5.0
        out += [dict(label=name, segment=[k * step + shift, (k + 1) * step + shift]) for k in range(6)]
    return out + [dict(label="NotInTheList", segment=[1.0, 4.0])]


def _save_checkpoints(recipe, config, dev, directory):
    os.makedirs(directory, exist_ok=True)
    for epoch in (1, 2):
        torch.manual_seed(100 + epoch)
        torch.save(recipe.build(config, dev).state_dict(), os.path.join(directory, f"checkpoint-{epoch}.ckpt"))


def _host_map(recipe, config, dev, directory, detect_all, gt_file, known, tious, dataset, subset, version, tmp_path):
    """{epoch: (mAP over the known classes, npos max)} by the host route."""
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
                            tiou_thresholds=np.asarray(tious), dataset=dataset, openset=True, ood_threshold=None, device='cpu')
        ap = det.evaluate('AP')[2]
        assert (ap[:, -1] == 0).all()                       # the '__unknown__' column: no detection carries that label
        npos = int(np.bincount(det.ground_truth['label'])[1:].max())
        out[epoch] = (ap[:, :-1].mean(axis=1), npos, sum(len(v) for v in results.values()))
    return out


def _check_map(map_file, result, want, capsys, rerun):
    from opental_amd.evaluation.table_ap import tolerance
    on_disk = json.load(open(map_file))
    assert on_disk == json.loads(json.dumps(result)) and sorted(on_disk) == ['1', '2', 'best']
    for epoch in (1, 2):
        mAP, npos, ndet = want[epoch]
        got = np.array(on_disk[str(epoch)]['mAP'])
        tol = tolerance(npos)
        with capsys.disabled():
            print("epoch", epoch, "detections", ndet, "npos", npos, "mAP", got, "max |dmAP|", float(np.abs(got - mAP).max()),
                  "tolerance", tol)
        assert ndet > 0 and got.shape == mAP.shape and tol < 1e-12
        assert np.abs(got - mAP).max() <= tol
        assert abs(on_disk[str(epoch)]['average_mAP'] - mAP.mean()) <= tol
    averages = [on_disk[str(e)]['average_mAP'] for e in (1, 2)]
    assert max(averages) > 0                                # the comparison is not one of zeros
    assert on_disk['best'] == (1 if averages[0] >= averages[1] else 2)
    # a second invocation finds both epochs in the file and scores nothing
    capsys.readouterr()
    mtime = os.path.getmtime(map_file)
    map_file2, result2 = rerun()
    text = capsys.readouterr().out
    assert (map_file2, result2) == (map_file, result) and text.count("skipped") == 2
    assert os.path.getmtime(map_file) == mtime


def test_thumos14_driver_equals_the_host_route(tmp_path, capsys, monkeypatch):
    from make_synthetic_thumos import CLASSES, make
    from opental_amd.common import config as C
    from opental_amd.common.thumos_dataset import get_class_index_map, get_video_info
    from opental_amd.thumos14 import score_checkpoints as S, test as T
    data = tmp_path / "data"
    yaml_path = make(str(data), videos=1, frames=100, size=96, test_videos=0)
    rs = np.random.RandomState(5)
    names = [f"video_test_{v:07d}" for v in range(4)]
    rows = ["video,fps,sample_fps,count,sample_count"]
    database = {}
    for v, name in enumerate(names):
        np.save(str(data / "test_npy" / (name + ".npy")), rs.randint(0, 256, (300, 96, 96, 3)).astype(np.uint8))
        rows.append(f"{name},30.0,10.0,900,300")
        database[name] = dict(subset="test", duration=30.0, annotations=_annotations([n for _, n in CLASSES], v, 4, 30.0))
    (data / "test_info.csv").write_text("\n".join(rows) + "\n")
    gt_file, known, run_dir = str(data / "gt_dense.json"), str(data / "classes.txt"), str(tmp_path / "run")
    json.dump(dict(database=database), open(gt_file, "w"))
    argv = [yaml_path, '--open_set', '--split', '0', '--checkpoint_path', run_dir, '--gt', gt_file, '--known', known]
    config = C.get_config(argv[:6])
    dev = torch.device("cuda", 0)
    _save_checkpoints(S.RECIPE, config, dev, run_dir)
    map_file, result = S.main(argv)
    assert map_file == os.path.join(run_dir, "checkpoint_map.json")
    te, ds = config['testing'], config['dataset']['testing']
    infos = get_video_info(ds['video_info_path'])
    assert list(infos) == names
    detect_all = lambda net: T.test(net, infos, ds['video_data_path'], get_class_index_map(known)[1], ds['clip_length'],
                                    ds['clip_stride'], ds['crop_size'], te['conf_thresh'], te['top_k'], te['nms_sigma'], device=dev)
    want = _host_map(S.RECIPE, config, dev, run_dir, detect_all, gt_file, known, S.RECIPE.tious, 'thumos14', ['test'], "THUMOS14",
                     tmp_path)
    assert len(result['1']['mAP']) == 5
    monkeypatch.setattr(S.RECIPE, "build", lambda *a: pytest.fail("a skipped epoch must not build the network"))
    _check_map(map_file, result, want, capsys, lambda: S.main(argv))


def test_anet_driver_equals_the_host_route(tmp_path, capsys, monkeypatch):
    from make_synthetic_anet import make
    from opental_amd.anet import score_checkpoints as S, test as AT
    from opental_amd.common import config as C
    root = tmp_path / "anet"
    yaml_path = make(str(root), videos=2, size=96)
    cfg = yaml.load(open(yaml_path).read(), Loader=yaml.FullLoader)
    cfg['testing']['conf_thresh'] = 0.0005      # a random network spreads its score over 150 classes: below the recipe's 0.01
    with open(yaml_path, "w") as f:
        yaml.dump(cfg, f)
    rs = np.random.RandomState(9)
    class_names = [f"class_{i}" for i in range(150)]
    info, database = {}, {}
    for v in range(2):
        name = f"v_synth{v:05d}"
        np.save(str(root / "train_val_npy" / (name + ".npy")), rs.randint(0, 256, (768, 96, 96, 3)).astype(np.uint8))
        info[name] = dict(subset="validation", fps=10.0, frame_num=768, duration=76.8, annotations=[])
        database[name[2:]] = dict(subset="validation", duration=76.8, annotations=_annotations(class_names, v, 2, 76.8))
    json.dump(info, open(root / "video_info.json", "w"))
    gt_file, known, run_dir = str(root / "gt_dense.json"), str(root / "action_known.txt"), str(tmp_path / "run")
    json.dump(dict(database=database), open(gt_file, "w"))
    argv = [yaml_path, '--open_set', '--split', '0', '--checkpoint_path', run_dir, '--gt', gt_file, '--known', known]
    config = C.get_config(argv[:6])
    dev = torch.device("cuda", 0)
    _save_checkpoints(S.RECIPE, config, dev, run_dir)
    map_file, result = S.main(argv)
    te, t = config['testing'], config['dataset']['testing']
    detect_all = lambda net: AT.testing(net, list(info), info, t['video_mp4_path'], AT.get_class_names(known), t['clip_length'],
                                        t['crop_size'], te['conf_thresh'], te['top_k'], te['nms_sigma'], device=dev)
    want = _host_map(S.RECIPE, config, dev, run_dir, detect_all, gt_file, known, S.RECIPE.tious, 'anet', ['validation'],
                     "ActivityNet-v1.3", tmp_path)
    assert len(result['1']['mAP']) == 10
    monkeypatch.setattr(S.RECIPE, "build", lambda *a: pytest.fail("a skipped epoch must not build the network"))
    _check_map(map_file, result, want, capsys, lambda: S.main(argv))
