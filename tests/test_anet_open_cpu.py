"""CPU: the ActivityNet1.3 open-set drivers -- opental_amd.anet.threshold (video selection, the rank merge, the result file
and its re-use) and opental_amd.anet.eval_open (against direct ANETdetection(dataset='anet') calls, and the text files)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from det_table_cases import make_case

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ----------------------------------------------------------------------------- threshold driver
def test_video_selection(tmp_path):
    from opental_amd.anet.threshold import select_videos
    order = ['v_m', 'v_a', 'v_z', 'v_c', 'v_k', 'v_b']
    subset = dict(v_m='training', v_a='validation', v_z='training', v_c='training', v_k='testing', v_b='training')
    info = {n: {'subset': subset[n], 'duration': 10.0, 'fps': 5.0} for n in order}
    (tmp_path / 'info.json').write_text(json.dumps(info))
    npy = tmp_path / 'npy'
    npy.mkdir()
    for n in ('v_b', 'v_a', 'v_z', 'v_m', 'v_k', 'v_other'):        # v_c is not on disk; v_other is not in the file
        np.save(npy / (n + '.npy'), np.zeros(1, np.uint8))
    (npy / 'v_c.txt').write_text('not a video')
    names, infos = select_videos(str(tmp_path / 'info.json'), str(npy))
    assert names == ['v_m', 'v_z', 'v_b']                            # training only, on disk only, file order
    assert set(infos) == {'v_m', 'v_z', 'v_c', 'v_b'}


def _fake_run(n_videos=7, K=4, top_k=6):
    rows, counts, durations = make_case(n_videos, K, top_k, 5, seed=11)
    names = ['v_%02d' % v for v in range(n_videos)]
    infos = {n: {'duration': float(durations[v]), 'fps': 5.0} for v, n in enumerate(names)}
    index = {n: v for v, n in enumerate(names)}

    def detect(part):
        sel = [index[n] for n in part]
        return torch.from_numpy(rows[sel]), torch.from_numpy(counts[sel])
    return names, infos, detect, (rows, counts, durations)


@pytest.mark.parametrize("scoring", ['uncertainty', 'half_au'])
def test_rank_merge_equals_the_one_rank_result(scoring):
    from opental_amd.anet.test import get_video_prediction
    from opental_amd.anet.threshold import known_scores, merge_scores
    from opental_amd.common.det_table import threshold_from_scores
    from opental_amd.thumos14.test import ood_threshold
    names, infos, detect, (rows, counts, durations) = _fake_run()
    one, one_res = known_scores(detect, names, infos, scoring, batch_videos=3, keep=True)
    dicts = {n[2:]: get_video_prediction(torch.from_numpy(rows[v]), torch.from_numpy(counts[v]), float(durations[v]))
             for v, n in enumerate(names)}
    assert one_res == dicts and one.numel() == sum(len(p) for p in dicts.values()) > 50
    want = ood_threshold(dicts, scoring)
    assert threshold_from_scores(one) == want
    for world in (2, 3):
        parts = [known_scores(detect, names, infos, scoring, batch_videos=2, rank=r, world=world, keep=True) for r in range(world)]
        merged = merge_scores([p[0].numpy() for p in parts])        # what travels between ranks is a numpy array
        assert merged.dtype == torch.float64 and merged.numel() == one.numel()
        assert torch.equal(torch.sort(merged).values, torch.sort(one).values)
        assert threshold_from_scores(merged) == want
        res = {}
        for _, r in parts:
            res.update(r)
        assert res == dicts
    # without `keep` no dict is built
    assert known_scores(detect, names, infos, scoring)[1] == {}
    assert merge_scores([]).numel() == 0


def test_threshold_file_is_written_whole(tmp_path):
    from opental_amd.anet.threshold import read_threshold_file, write_threshold_file
    out = tmp_path / 'deep' / 'er' / 'thr.json'
    assert read_threshold_file(str(out)) is None
    write_threshold_file(str(out), 0.25)
    assert json.loads(out.read_text()) == {"version": "ActivityNet-v1.3", "results": {}, "external_data": {"threshold": 0.25}}
    write_threshold_file(str(out), 0.5, {'a': [{'label': 1, 'score': 0.5, 'segment': [0.0, 1.0], 'uncertainty': 0.1, 'actionness': 0.9}]})
    data = json.loads(out.read_text())
    assert data['external_data'] == {'threshold': 0.5} and list(data['results']) == ['a']
    assert os.listdir(out.parent) == ['thr.json']                   # the temporary file was moved, not copied
    assert read_threshold_file(str(out)) == 0.5
    (tmp_path / 'plain.json').write_text(json.dumps({"version": "ActivityNet-v1.3", "results": {}, "external_data": {}}))
    assert read_threshold_file(str(tmp_path / 'plain.json')) is None    # a detection file of anet.test carries no threshold


def test_write_json_replaces_the_file_whole(tmp_path):
    from opental_amd.common.driver import write_json
    out = tmp_path / 'not' / 'there' / 'yet' / 'res.json'
    obj = {"version": "THUMOS14", "results": {"v": [{"label": "A", "score": 0.5, "segment": [0.0, 1.5]}]}, "external_data": {}}
    write_json(str(out), obj)
    assert json.loads(out.read_text()) == obj
    assert os.listdir(out.parent) == ['res.json']                   # no temporary file is left behind
    write_json(str(out), {"results": {}})                           # an existing file is replaced
    assert json.loads(out.read_text()) == {"results": {}}
    assert os.listdir(out.parent) == ['res.json']


def test_split_flags_on_each_drivers_flag_set():
    from opental_amd.common.driver import split_flags
    base = ['cfg.yaml', '--open_set', '--split', '0']
    # thumos14.test / test_openmax: --random_init and --evaluate GT KNOWN, anywhere on the line
    flags, options = ('--random_init',), {'--evaluate': (2, None)}
    found, rest = split_flags(['cfg.yaml', '--evaluate', 'gt.json', 'known.txt', '--open_set', '--random_init', '--split', '0'],
                              flags, options)
    assert found == {'--random_init': True, '--evaluate': ('gt.json', 'known.txt')} and rest == base
    assert split_flags(base, flags, options) == ({'--random_init': False, '--evaluate': None}, base)
    for line in (base + ['--evaluate'], base + ['--evaluate', 'gt.json']):
        with pytest.raises(ValueError, match='--evaluate takes 2 values'):
            split_flags(line, flags, options)
    # thumos14.test_cross_data: three valued options with defaults
    options = {'--anet_info': (1, 'info.json'), '--anet_npy': (1, 'npy'), '--anet_overlap': (1, 'overlap.txt')}
    found, rest = split_flags(base[:1] + ['--anet_npy', '/data/npy', '--random_init'] + base[1:] + ['--anet_overlap', 'o.txt'],
                              flags, options)
    assert found == {'--random_init': True, '--anet_info': 'info.json', '--anet_npy': '/data/npy', '--anet_overlap': 'o.txt'}
    assert rest == base
    with pytest.raises(ValueError, match='--anet_info takes 1 value'):
        split_flags(base + ['--anet_info'], flags, options)
    # thumos14.threshold / anet.test: one flag; what the config parser reads (--ood_scoring S) passes through
    line = base + ['--ood_scoring', 'uncertainty', '--output_json', 'thr.json']
    assert split_flags(line + ['--random_init'], ('--random_init',)) == ({'--random_init': True}, line)
    # anet.threshold: two flags
    found, rest = split_flags(['--keep_detections'] + line, ('--random_init', '--keep_detections'))
    assert found == {'--random_init': False, '--keep_detections': True} and rest == line
    assert split_flags([], ('--random_init',)) == ({'--random_init': False}, [])


def test_existing_threshold_is_reused_without_the_gpu(tmp_path, monkeypatch, capsys):
    sys.path.insert(0, os.path.join(REPO, 'tools'))
    try:
        from make_synthetic_anet import make
    finally:
        sys.path.pop(0)
    from opental_amd.anet import threshold as TH
    yaml_path = make(str(tmp_path / 'data'), videos=1, size=8)
    out = tmp_path / 'data' / 'output' / 'thr.json'
    TH.write_threshold_file(str(out), 0.123456789)

    def refuse(*a, **k):
        raise AssertionError("the GPU was touched")
    for name in ('set_device', 'init', '_lazy_init', 'current_device', 'is_available', 'device_count'):
        monkeypatch.setattr(torch.cuda, name, refuse)
    got = TH.main([yaml_path, '--open_set', '--split', '0', '--ood_scoring', 'uncertainty', '--output_json', 'thr.json',
                   '--random_init', '--keep_detections'])
    assert got == (str(out), 0.123456789)
    text = capsys.readouterr().out
    assert 'already exist' in text and 'The threshold is: 0.123456789000' in text


# ----------------------------------------------------------------------------- evaluation driver
CLASSES = ['Archery', 'Playing water polo', 'Zumba', 'Tango']         # one name per line, names with blanks


def _anet_files(root, split, seed):
    """A tiny ActivityNet-style ground truth (open: some annotations carry a class outside the known list; closed: known
    classes only), a prediction file of anet.test's layout and the class list, under root/split_<split>/."""
    rs = np.random.RandomState(seed)
    d = root / ('split_%d' % split)
    d.mkdir(parents=True)
    (d / 'action_known.txt').write_text(''.join(c + '\n' for c in CLASSES))
    db_open, db_closed, results = {}, {}, {}
    for v in range(8):
        vid = 'vid%02d' % v
        annos_open, annos_closed, dets = [], [], []
        t = 0.0
        for j in range(5):
            s = t + float(rs.uniform(1.0, 4.0))
            e = s + float(rs.uniform(4.0, 12.0))
            t = e
            known = (v + j) % 3 != 0
            label = CLASSES[(v + j) % 4]
            annos_open.append({'label': label if known else 'Unseen activity %d' % (j % 2), 'segment': [s, e]})
            annos_closed.append({'label': label, 'segment': [s, e]})
            for _ in range(int(rs.randint(1, 4))):
                js, je = s + float(rs.normal(0, 0.8)), e + float(rs.normal(0, 0.8))
                u = float(np.float32(np.clip(rs.normal(0.3 if known else 0.6, 0.2), 0.01, 0.99)))
                dets.append({'label': label if rs.rand() < 0.8 else CLASSES[int(rs.randint(4))],
                             'score': float(np.float32(rs.uniform(0.05, 0.95))), 'segment': [max(0.0, js), je],
                             'uncertainty': u, 'actionness': float(np.float32(rs.uniform(0.5, 1.0)))})
        for _ in range(3):
            s = float(rs.uniform(0, t))
            dets.append({'label': CLASSES[int(rs.randint(4))], 'score': float(np.float32(rs.uniform(0.01, 0.3))),
                         'segment': [s, s + float(rs.uniform(1, 5))], 'uncertainty': float(np.float32(rs.uniform(0.2, 0.9))),
                         'actionness': float(np.float32(rs.uniform(0.5, 1.0)))})
        order = rs.permutation(len(dets))
        results[vid] = [dets[i] for i in order]
        db_open[vid] = {'subset': 'validation', 'duration': t + 5.0, 'annotations': annos_open}
        db_closed[vid] = {'subset': 'validation', 'duration': t + 5.0, 'annotations': annos_closed}
    # a training video must not count: the subset is ['validation']
    for db in (db_open, db_closed):
        db['train00'] = {'subset': 'training', 'duration': 30.0, 'annotations': [{'label': CLASSES[0], 'segment': [1.0, 9.0]}]}
    results['train00'] = [{'label': CLASSES[0], 'score': 0.9, 'segment': [1.0, 9.0], 'uncertainty': 0.1, 'actionness': 0.9}]
    (d / 'known_gt.json').write_text(json.dumps({'database': db_open}))
    (d / 'closed_gt.json').write_text(json.dumps({'database': db_closed}))
    (d / 'detection_results.json').write_text(json.dumps({'version': 'ActivityNet-v1.3', 'results': results, 'external_data': {}}))
    return d


@pytest.fixture(scope="module")
def anet_root(tmp_path_factory):
    root = tmp_path_factory.mktemp('anet_eval')
    return root, [_anet_files(root, s, seed=40 + s) for s in (0, 1)]


def _patterns(root, gt):
    p = str(root / 'split_{id:d}')
    return [os.path.join(p, 'detection_results.json'), os.path.join(p, gt), '--cls_idx_known', os.path.join(p, 'action_known.txt')]


def test_eval_open_equals_direct_evaluator_calls(anet_root, capsys):
    from opental_amd.anet import eval_open
    from opental_amd.evaluation.eval_detection import ANETdetection
    root, dirs = anet_root
    got = eval_open.main(_patterns(root, 'known_gt.json') + ['--all_splits', '0', '1', '--open_set', '--ood_scoring', 'uncertainty'])
    printed = capsys.readouterr().out
    tious = np.linspace(0.5, 0.95, 10)
    for split, d in enumerate(dirs):
        det = ANETdetection(ground_truth_filename=str(d / 'known_gt.json'), prediction_filename=str(d / 'detection_results.json'),
                            cls_idx_detection=str(d / 'action_known.txt'), subset=['validation'], openset=True,
                            ood_scoring='uncertainty', tiou_thresholds=tious, dataset='anet')
        assert 'train00' not in det.video_lst and len(det.prediction['score']) > 80
        det.pre_evaluate()
        auc_roc, auc_pr, far_95 = det.evaluate(type='AUC')
        osdr = det.evaluate(type='OSDR')
        assert 0.0 < auc_roc[0] < 1.0 and osdr[0] > 0.0             # both kinds of ground truth were matched
        for key, want in (('far_95', far_95), ('auc_roc', auc_roc), ('auc_pr', auc_pr), ('osdr', osdr)):
            assert np.array_equal(got[split][key], want), (split, key)
        lines = (d / 'eval_open.txt').read_text().splitlines()
        assert len(lines) == 11
        assert lines[0] == (f"tIoU={tious[0]}: far@95={far_95[0]:.5f}, auc_roc={auc_roc[0]:.5f}, auc_pr={auc_pr[0]:.5f}, "
                            f"osdr={osdr[0]:.5f}")
        assert lines[-1] == (f"Average FAR@95: {far_95.mean():.5f}, Average AUC_ROC: {auc_roc.mean():.5f}, "
                             f"Average AUC_PR: {auc_pr.mean():.5f}, Average OSDR: {osdr.mean():.5f}")
    assert printed.count('FAR@95(tIoU=') == 10 and 'Average OSDR = ' in printed


def test_eval_closed_set_equals_direct_evaluator_calls(anet_root, capsys):
    from opental_amd.anet import eval_open
    from opental_amd.evaluation.eval_detection import ANETdetection
    root, dirs = anet_root
    got = eval_open.main(_patterns(root, 'closed_gt.json') + ['--all_splits', '0', '1'])
    printed = capsys.readouterr().out
    tious = np.linspace(0.5, 0.95, 10)
    for split, d in enumerate(dirs):
        det = ANETdetection(ground_truth_filename=str(d / 'closed_gt.json'), prediction_filename=str(d / 'detection_results.json'),
                            cls_idx_detection=str(d / 'action_known.txt'), subset=['validation'], openset=False,
                            tiou_thresholds=tious, dataset='anet')
        mAPs, average_mAP, _ = det.evaluate(type='AP')
        assert mAPs[0] > 0.0
        assert np.array_equal(got[split]['mAP'], mAPs) and got[split]['average_mAP'] == average_mAP
        lines = (d / 'eval.txt').read_text().splitlines()
        assert len(lines) == 11 and lines[0] == f"tIoU={tious[0]}: mAP={mAPs[0]:.5f}" and lines[-1] == f"Average mAP: {average_mAP:.5f}"
    assert printed.count('mAP(tIoU=') == 10 and 'Average mAP = ' in printed


def test_tious_flag_selects_the_stale_list(anet_root):
    from opental_amd.anet import eval_open
    root, dirs = anet_root
    got = eval_open.main(_patterns(root, 'closed_gt.json') + ['--all_splits', '0', '--tious', '0.1', '0.2', '0.3', '0.4', '0.5'])
    assert got[0]['mAP'].shape == (5,)
    assert (dirs[0] / 'eval.txt').read_text().splitlines()[0].startswith('tIoU=0.1: mAP=')
    assert np.array_equal(eval_open.default_tious(), np.linspace(0.5, 0.95, 10))
