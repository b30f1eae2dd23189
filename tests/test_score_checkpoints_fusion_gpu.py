"""GPU: python -m opental_amd.thumos14.score_checkpoints --fusion on two randomly initialised rgb checkpoints, one flow
checkpoint and two synthetic videos (rgb and flow .npy of 300 frames): checkpoint_map_fusion.json against the host route on the
same checkpoints -- thumos14.test.test(net, ..., flow_net=, flow_data_path=) -> results_json ->
ANETdetection(device='cpu').evaluate('AP') -- the skipping of epochs already scored with this partner, their re-scoring with
another one, and checkpoint_map.json left alone.

Tolerance (table_ap.tolerance): |dAP| <= 4 npos 2^-53 per class with the ground truth's largest npos, the bound of
tests/test_score_checkpoints_gpu.py, whose dense ground truth (every class tiles half a minute of the videos) is used too, so
that detections of random networks match some of it and the comparison is not one of zeros."""
import json
import os
import shutil
import sys

import numpy as np
import pytest
import torch

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


def test_thumos14_fusion_driver_equals_the_host_route(tmp_path, capsys, monkeypatch):
    from make_synthetic_thumos import CLASSES, make
    from opental_amd.common import config as C
    from opental_amd.common.detect import results_json
    from opental_amd.common.thumos_dataset import get_class_index_map, get_video_info
    from opental_amd.evaluation.eval_detection import ANETdetection
    from opental_amd.evaluation.table_ap import tolerance
    from opental_amd.thumos14 import score_checkpoints as S, test as T
    data = tmp_path / "data"
    yaml_path = make(str(data), videos=1, frames=100, size=96, test_videos=0)
    flow_dir = data / "test_flow_npy"
    os.makedirs(str(flow_dir))
    rs = np.random.RandomState(5)
    names = [f"video_test_{v:07d}" for v in range(2)]
    rows, database = ["video,fps,sample_fps,count,sample_count"], {}
    for v, name in enumerate(names):
        np.save(str(data / "test_npy" / (name + ".npy")), rs.randint(0, 256, (300, 96, 96, 3)).astype(np.uint8))
        np.save(str(flow_dir / (name + ".npy")), rs.randint(0, 256, (300, 96, 96, 2)).astype(np.uint8))
        rows.append(f"{name},30.0,10.0,900,300")
        database[name] = dict(subset="test", duration=30.0, annotations=_annotations([n for _, n in CLASSES], v, 2, 30.0))
    (data / "test_info.csv").write_text("\n".join(rows) + "\n")
    gt_file, known, run_dir = str(data / "gt_dense.json"), str(data / "classes.txt"), str(tmp_path / "run")
    json.dump(dict(database=database), open(gt_file, "w"))
    base = [yaml_path, '--open_set', '--split', '0', '--checkpoint_path', run_dir, '--gt', gt_file, '--known', known]
    config = C.get_config(base[:6])
    dev = torch.device("cuda", 0)
    os.makedirs(run_dir)
    for epoch in (1, 2):
        torch.manual_seed(100 + epoch)
        torch.save(S.RECIPE.build(config, dev).state_dict(), os.path.join(run_dir, f"checkpoint-{epoch}.ckpt"))
    partner_file = str(tmp_path / "flow" / "checkpoint-7.ckpt")
    os.makedirs(os.path.dirname(partner_file))
    torch.manual_seed(207)
    flow_net = S.RECIPE.partner_build(config, dev)
    assert flow_net.backbone._model.Conv3d_1a_7x7.conv3d.weight.shape[1] == 2
    # Randomly initialised actionness heads lean negative (logits -2.3 .. 1.1 here), and the average of two such networks has
    # no anchor left with actionness > 0.5: no detection at all.  The flow checkpoint's two actionness biases are raised so
    # that the fused actionness straddles 0.5 and the comparison is not one of empty results.  Their segments are short as
    # well (loc = exp(head): 0.1 .. 10 frames a side, averaged about a quarter of a second wide) against ground-truth segments
    # of five seconds: no detection reaches tIoU 0.3.  The flow checkpoint's loc bias is raised by 3.5 (x 33), which spreads the
    # fused widths over roughly half a second to eight seconds.
    with torch.no_grad():
        flow_net.coarse_pyramid_detection.loc_head.conv1d.bias.add_(3.5)
        flow_net.coarse_pyramid_detection.actionness_head.conv1d.bias.add_(2.0)
        flow_net.coarse_pyramid_detection.prop_actionness_head.conv1d.bias.add_(2.0)
    torch.save(flow_net.state_dict(), partner_file)
    argv = base + ['--fusion', '--partner_checkpoint', partner_file, '--partner_data', str(flow_dir)]

    map_file, result = S.main(argv)
    assert map_file == os.path.join(run_dir, "checkpoint_map_fusion.json")
    on_disk = json.load(open(map_file))
    assert on_disk == json.loads(json.dumps(result)) and sorted(on_disk) == ['1', '2', 'best']

    # the host route on the same three checkpoints
    te, ds = config['testing'], config['dataset']['testing']
    infos = get_video_info(ds['video_info_path'])
    assert list(infos) == names
    net = S.RECIPE.build(config, dev)
    averages = []
    for epoch in (1, 2):
        net.load_state_dict(torch.load(os.path.join(run_dir, f"checkpoint-{epoch}.ckpt"), map_location='cpu'))
        with torch.no_grad():
            results = T.test(net, infos, ds['video_data_path'], get_class_index_map(known)[1], ds['clip_length'], ds['clip_stride'],
                             ds['crop_size'], te['conf_thresh'], te['top_k'], te['nms_sigma'], device=dev, flow_net=flow_net,
                             flow_data_path=str(flow_dir))
        pred_file = str(tmp_path / f"pred_{epoch}.json")
        json.dump(results_json(results, version="THUMOS14"), open(pred_file, "w"))
        det = ANETdetection(ground_truth_filename=gt_file, prediction_filename=pred_file, cls_idx_detection=known, subset=['test'],
                            tiou_thresholds=np.asarray(S.RECIPE.tious), dataset='thumos14', openset=True, ood_threshold=None,
                            device='cpu')
        ap = det.evaluate('AP')[2]
        assert (ap[:, -1] == 0).all()                       # the '__unknown__' column: no detection carries that label
        want = ap[:, :-1].mean(axis=1)
        npos = int(np.bincount(det.ground_truth['label'])[1:].max())
        ndet = sum(len(v) for v in results.values())
        entry = on_disk[str(epoch)]
        got, tol = np.array(entry['mAP']), tolerance(npos)
        with capsys.disabled():
            print("epoch", epoch, "detections", ndet, "npos", npos, "mAP", got, "max |dmAP|", float(np.abs(got - want).max()),
                  "tolerance", tol)
        assert ndet > 0 and got.shape == want.shape == (5,) and tol < 1e-12
        assert np.abs(got - want).max() <= tol
        assert abs(entry['average_mAP'] - want.mean()) <= tol
        assert entry['partner_checkpoint'] == partner_file
        averages.append(entry['average_mAP'])
    assert max(averages) > 0                                # the comparison is not one of zeros
    assert on_disk['best'] == (1 if averages[0] >= averages[1] else 2)

    # a second invocation finds both epochs scored with this partner and builds nothing
    built = []
    build = S.RECIPE.build
    monkeypatch.setattr(S.RECIPE, "build", lambda *a: (built.append(1), build(*a))[1])
    capsys.readouterr()
    mtime = os.path.getmtime(map_file)
    assert S.main(argv) == (map_file, result)
    assert capsys.readouterr().out.count("skipped") == 2 and not built and os.path.getmtime(map_file) == mtime

    # another partner path (the same weights under another name): both epochs are scored again and say so
    other = str(tmp_path / "flow" / "checkpoint-8.ckpt")
    shutil.copy(partner_file, other)
    map_file2, result2 = S.main(argv[:argv.index('--partner_checkpoint') + 1] + [other] + argv[-2:])
    text = capsys.readouterr().out
    assert map_file2 == map_file and "skipped" not in text and built
    for epoch in ('1', '2'):
        assert result2[epoch]['partner_checkpoint'] == other
        assert result2[epoch]['mAP'] == result[epoch]['mAP']            # the same weights: the same numbers
    assert not os.path.exists(os.path.join(run_dir, "checkpoint_map.json"))
