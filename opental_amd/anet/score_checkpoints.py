"""python -m opental_amd.anet.score_checkpoints <yaml> [--open_set --split N] --gt GT.json --known KNOWN.txt \\
       [--epochs A B ...] [--tious ...] [--random_init] [--select KEY] \\
       [--open_metrics [--ood_threshold THR | --threshold_from_train [--threshold_videos N]] [--wi]]

The mAP of every saved epoch of the ActivityNet1.3 recipe on the validation videos, from detection tables on the device
(common/score_checkpoints.py): the network, video list, batches and thresholds of anet/test.py (`testing`: the validation
videos that exist on disk, batches of 4), segments clipped to the videos' durations as anet/threshold.py passes them to the
table, the `validation` subset of the ground truth (whose names carry no "v_"), tIoU 0.5 .. 0.95.  With --open_set
--open_metrics also AUROC, AUPR, FAR@95 and OSDR per tIoU (evaluation/table_open.py), the tables' `known` column by
--ood_scoring; --select KEY names what "best" goes by.  --threshold_from_train takes each epoch's known / unknown threshold from a
pass over the training videos (the list and arguments of anet/threshold.py; --threshold_videos N caps it) and --wi adds the
Wilderness Impact at it (evaluation/table_wi.py).  ActivityNet1.3 has no flow stream in this package: --fusion is refused."""
import json
import os

import numpy as np

from ..common import ops
from ..common.driver import load_net
from ..common.score_checkpoints import Recipe, run
from . import test as T

BATCH_CLIPS = 4         # anet.test.testing's default: its batches of videos and of clips
TRAIN_BATCH_VIDEOS = 8  # anet.threshold.thresholding's default batch_videos


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
    """Batches of BATCH_CLIPS videos; a state with a third member (the training split's) names its own batch size."""
    n, step = len(state[0]), state[2] if len(state) > 2 else BATCH_CLIPS
    return [list(range(i, min(i + step, n))) for i in range(0, n, step)]


def _table(net, config, state, positions, dev, scoring='uncertainty', npy_path=None):
    video_list, infos = state[:2]
    te, t = config['testing'], config['dataset']['testing']
    part = [video_list[p] for p in positions]
    vids = [T.prepare_data(npy_path or t['video_mp4_path'], n, t['crop_size'], dev) for n in part]
    rows, counts = T.detect_rows(net, vids, [float(infos[n]['fps']) for n in part], t['clip_length'], te['conf_thresh'],
                                 te['top_k'], te['nms_sigma'], BATCH_CLIPS)
    return ops.detection_table(rows, counts, [float(infos[n]['duration']) for n in part], scoring=scoring)


def _train_videos(config):
    """The list anet/threshold.py's `main` runs over (select_videos: the `training` videos that exist on disk), in
    `thresholding`'s batches of TRAIN_BATCH_VIDEOS videos."""
    from .threshold import select_videos
    tr = config['dataset']['training']
    video_list, infos = select_videos(tr['video_info_path'], tr['video_mp4_path'])
    return [n[2:] for n in video_list], (video_list, infos, TRAIN_BATCH_VIDEOS)


def _train_table(net, config, state, positions, dev, scoring='uncertainty'):
    """`_table` over the training split with anet.threshold.thresholding's arguments: the training .npy path, the testing
    clip length, crop and thresholds, clips in batches of BATCH_CLIPS, segments clipped to the durations."""
    return _table(net, config, state, positions, dev, scoring, config['dataset']['training']['video_mp4_path'])


RECIPE = Recipe('anet', ['validation'], np.linspace(0.5, 0.95, 10), _build, _videos, _batches, _table, _train_videos,
                _train_table)


def main(argv=None):
    import sys
    if '--fusion' in (sys.argv[1:] if argv is None else argv):
        raise SystemExit("score_checkpoints: ActivityNet1.3 has no flow stream (one rgb network per recipe): --fusion is not served")
    return run(RECIPE, argv)


if __name__ == '__main__':
    main()
