"""python -m opental_amd.anet.score_checkpoints <yaml> [--open_set --split N] --gt GT.json --known KNOWN.txt \\
       [--epochs A B ...] [--tious ...] [--random_init] [--open_metrics [--ood_threshold THR]] [--select KEY]

The mAP of every saved epoch of the ActivityNet1.3 recipe on the validation videos, from detection tables on the device
(common/score_checkpoints.py): the network, video list, batches and thresholds of anet/test.py (`testing`: the validation
videos that exist on disk, batches of 4), segments clipped to the videos' durations as anet/threshold.py passes them to the
table, the `validation` subset of the ground truth (whose names carry no "v_"), tIoU 0.5 .. 0.95.  With --open_set
--open_metrics also AUROC, AUPR, FAR@95 and OSDR per tIoU (evaluation/table_open.py), the tables' `known` column by
--ood_scoring; --select KEY names what "best" goes by."""
import json
import os

import numpy as np

from ..common import ops
from ..common.driver import load_net
from ..common.score_checkpoints import Recipe, run
from . import test as T

BATCH_CLIPS = 4         # anet.test.testing's default: its batches of videos and of clips


def _build(config, dev):
    from .BDNet import BDNet, model_cfg_from
    md, t = config['model'], config['dataset']['testing']
    return load_net(BDNet, dev, True, None, in_channels=md['in_channels'], frame_num=t['clip_length'],
                    use_edl=md.get('use_edl', False), cfg=model_cfg_from(config))


def _videos(config):
    t = config['dataset']['testing']
    with open(t['video_info_path']) as f:
        infos = {k: v for k, v in json.load(f).items() if v.get('subset', 'validation') == 'validation'}
    on_disk = {f[:-4] for f in os.listdir(t['video_mp4_path']) if f.endswith('.npy')}
    video_list = [n for n in infos if n in on_disk]
    return [n[2:] for n in video_list], (video_list, infos)


def _batches(config, state):
    n = len(state[0])
    return [list(range(i, min(i + BATCH_CLIPS, n))) for i in range(0, n, BATCH_CLIPS)]


def _table(net, config, state, positions, dev, scoring='uncertainty'):
    video_list, infos = state
    te, t = config['testing'], config['dataset']['testing']
    part = [video_list[p] for p in positions]
    vids = [T.prepare_data(t['video_mp4_path'], n, t['crop_size'], dev) for n in part]
    rows, counts = T.detect_rows(net, vids, [float(infos[n]['fps']) for n in part], t['clip_length'], te['conf_thresh'],
                                 te['top_k'], te['nms_sigma'], BATCH_CLIPS)
    return ops.detection_table(rows, counts, [float(infos[n]['duration']) for n in part], scoring=scoring)


RECIPE = Recipe('anet', ['validation'], np.linspace(0.5, 0.95, 10), _build, _videos, _batches, _table)


def main(argv=None):
    return run(RECIPE, argv)


if __name__ == '__main__':
    main()
