"""python -m opental_amd.thumos14.score_checkpoints <yaml> [--open_set --split N] --gt GT.json --known KNOWN.txt \\
       [--epochs A B ...] [--tious ...] [--random_init] [--select KEY] \\
       [--open_metrics [--ood_threshold THR | --threshold_from_train [--threshold_videos N]] [--wi]] \\
       [--fusion --partner_checkpoint PATH --partner_data DIR [--partner_train_data DIR]]

The mAP of every saved epoch of the THUMOS14 recipe on the test videos, from detection tables on the device
(common/score_checkpoints.py): the network, batches and thresholds of thumos14/test.py (`test`: batches of 8 videos), the
`test` subset of the ground truth, tIoU 0.3 .. 0.7.  With --open_set --open_metrics also AUROC, AUPR, FAR@95 and OSDR per tIoU
(evaluation/table_open.py), the tables' `known` column by --ood_scoring; --select KEY names what "best" goes by.  --threshold_from_train takes each epoch's known / unknown threshold from a
pass over the training videos (the list and arguments of thumos14/threshold.py) and --wi adds the Wilderness Impact at it
(evaluation/table_wi.py).  --fusion scores the epochs together with ONE checkpoint of the other stream (model.in_channels 3: the
epochs are rgb and --partner_checkpoint is a flow network, read from --partner_data; 2, with the flow yaml: the reverse) through
detect_batch's two-stream route, into checkpoint_map_fusion.json."""
from ..common import ops
from ..common.detect import prepare_data
from ..common.driver import load_net
from ..common.score_checkpoints import Recipe, run
from ..common.thumos_dataset import get_video_info
from . import test as T

BATCH_VIDEOS = 8        # thumos14.test.test's default


def _build(config, dev, in_channels=None):
    from .BDNet import BDNet, model_cfg_from
    md = config['model']
    return load_net(BDNet, dev, True, None, in_channels=in_channels or md['in_channels'], use_edl=md.get('use_edl', False),
                    use_rpl=False, cfg=model_cfg_from(config))


def _partner_channels(config):
    """The other stream's channel count: 2 (flow) beside rgb epochs, 3 (rgb) beside flow epochs."""
    listed = int(config['model']['in_channels'])
    if listed not in (2, 3):
        raise SystemExit("score_checkpoints: --fusion pairs an rgb (model.in_channels 3) with a flow (2) network, not %d" % listed)
    return 5 - listed


def _partner_build(config, dev):
    return _build(config, dev, _partner_channels(config))


def _videos(config):
    infos = get_video_info(config['dataset']['testing']['video_info_path'])
    return list(infos.keys()), infos


def _batches(config, infos):
    return [list(range(i, min(i + BATCH_VIDEOS, len(infos)))) for i in range(0, len(infos), BATCH_VIDEOS)]


def _table(net, config, infos, positions, dev, scoring='uncertainty', data_path=None, partner=None, partner_data=None):
    """partner + partner_data: the two-stream run, `net` and `partner` in the roles their channel counts name."""
    te, ds = config['testing'], config['dataset']['testing']
    names = list(infos.keys())
    part = [names[p] for p in positions]
    vids = [prepare_data(data_path or ds['video_data_path'], n, ds['crop_size'], dev) for n in part]
    flow = {}
    if partner is not None:
        partner_vids = [prepare_data(partner_data, n, ds['crop_size'], dev) for n in part]
        if _partner_channels(config) == 2:
            flow = dict(flow_net=partner, flow_videos=partner_vids)
        else:                                   # the listed epochs are the flow stream's
            net, vids, flow = partner, partner_vids, dict(flow_net=net, flow_videos=vids)
    rows, counts, _, _ = T.detect_batch(net, vids, [float(infos[n]['sample_fps']) for n in part], ds['clip_length'],
                                        ds['clip_stride'], te['conf_thresh'], te['top_k'], te['nms_sigma'], **flow)
    return ops.detection_table(rows, counts, scoring=scoring)


def _fusion_table(net, partner, partner_data, config, infos, positions, dev, scoring='uncertainty', train=False):
    """`_table` (train: `_train_table`) through the two-stream pipeline, the partner's videos read from `partner_data`."""
    data_path = config['dataset']['training']['video_data_path'] if train else None
    return _table(net, config, infos, positions, dev, scoring, data_path, partner, partner_data)


def _train_videos(config):
    """The list thumos14/threshold.py's `main` runs over: the TRAINING videos."""
    infos = get_video_info(config['dataset']['training']['video_info_path'])
    return list(infos.keys()), infos


def _train_table(net, config, infos, positions, dev, scoring='uncertainty'):
    """`_table` over the training split as thumos14/threshold.py's `main` passes it to `thresholding`: the training data path
    with the testing clip length, stride, crop and thresholds."""
    return _table(net, config, infos, positions, dev, scoring, config['dataset']['training']['video_data_path'])


RECIPE = Recipe('thumos14', ['test'], [0.3, 0.4, 0.5, 0.6, 0.7], _build, _videos, _batches, _table, _train_videos, _train_table,
                _partner_build, _fusion_table)


def main(argv=None):
    return run(RECIPE, argv)


if __name__ == '__main__':
    main()
