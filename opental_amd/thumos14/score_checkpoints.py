"""python -m opental_amd.thumos14.score_checkpoints <yaml> [--open_set --split N] --gt GT.json --known KNOWN.txt \\
       [--epochs A B ...] [--tious ...] [--random_init] [--select KEY] \\
       [--open_metrics [--ood_threshold THR | --threshold_from_train [--threshold_videos N]] [--wi]]

The mAP of every saved epoch of the THUMOS14 recipe on the test videos, from detection tables on the device
(common/score_checkpoints.py): the network, batches and thresholds of thumos14/test.py (`test`: batches of 8 videos), the
`test` subset of the ground truth, tIoU 0.3 .. 0.7.  With --open_set --open_metrics also AUROC, AUPR, FAR@95 and OSDR per tIoU
(evaluation/table_open.py), the tables' `known` column by --ood_scoring; --select KEY names what "best" goes by.  --threshold_from_train takes each epoch's known / unknown threshold from a
pass over the training videos (the list and arguments of thumos14/threshold.py) and --wi adds the Wilderness Impact at it
(evaluation/table_wi.py)."""
from ..common import ops
from ..common.detect import prepare_data
from ..common.driver import load_net
from ..common.score_checkpoints import Recipe, run
from ..common.thumos_dataset import get_video_info
from . import test as T

BATCH_VIDEOS = 8        # thumos14.test.test's default


def _build(config, dev):
    from .BDNet import BDNet, model_cfg_from
    md = config['model']
    return load_net(BDNet, dev, True, None, in_channels=md['in_channels'], use_edl=md.get('use_edl', False), use_rpl=False,
                    cfg=model_cfg_from(config))


def _videos(config):
    infos = get_video_info(config['dataset']['testing']['video_info_path'])
    return list(infos.keys()), infos


def _batches(config, infos):
    return [list(range(i, min(i + BATCH_VIDEOS, len(infos)))) for i in range(0, len(infos), BATCH_VIDEOS)]


def _table(net, config, infos, positions, dev, scoring='uncertainty', data_path=None):
    te, ds = config['testing'], config['dataset']['testing']
    names = list(infos.keys())
    part = [names[p] for p in positions]
    vids = [prepare_data(data_path or ds['video_data_path'], n, ds['crop_size'], dev) for n in part]
    rows, counts, _, _ = T.detect_batch(net, vids, [float(infos[n]['sample_fps']) for n in part], ds['clip_length'],
                                        ds['clip_stride'], te['conf_thresh'], te['top_k'], te['nms_sigma'])
    return ops.detection_table(rows, counts, scoring=scoring)


def _train_videos(config):
    """The list thumos14/threshold.py's `main` runs over: the TRAINING videos."""
    infos = get_video_info(config['dataset']['training']['video_info_path'])
    return list(infos.keys()), infos


def _train_table(net, config, infos, positions, dev, scoring='uncertainty'):
    """`_table` over the training split as thumos14/threshold.py's `main` passes it to `thresholding`: the training data path
    with the testing clip length, stride, crop and thresholds."""
    return _table(net, config, infos, positions, dev, scoring, config['dataset']['training']['video_data_path'])


RECIPE = Recipe('thumos14', ['test'], [0.3, 0.4, 0.5, 0.6, 0.7], _build, _videos, _batches, _table, _train_videos, _train_table)


def main(argv=None):
    return run(RECIPE, argv)


if __name__ == '__main__':
    main()
