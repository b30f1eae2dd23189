"""python -m opental_amd.anet.test_openmax <anet_softmax.yaml> --open_set --split N [--random_init] [--refined_feature]

The OpenMax baseline of the ActivityNet1.3 recipe on MI355X: the statistics pass, the Weibull fits and the inference path.
The reference has no such script (its OpenMax runs for THUMOS14 only, AFSD/thumos14/test_openmax.py), so this docstring
defines the behaviour, on the model of thumos14/test_openmax.py and anet/threshold.py.

Network.  The Softmax baseline's model and checkpoint (anet_softmax.yaml: 151 logits, class 0 = background): no training.
model.os_head or model.use_edl set raises NotImplementedError.

Statistics pass.
  * videos: the `training` videos of dataset.training.video_info_path that have an .npy in dataset.training.video_mp4_path
    and at least one valid annotation -- common.anet_dataset.split_videos, the training set itself.  Each is ONE
    centre-cropped clip of clip_length (768) frames at offset 0, a shorter video padded as anet.test pads it (127.5 before
    the normalisation = 0.0); eval mode, get_feat=True, `batch_clips` videos per forward pass;
  * positive anchors are those the ActivityNet training loss calls positive: anet.multisegment_loss.MultiSegmentLoss.match
    with training.piou and the module's per-level regression bounds -- that code is called, not restated.  conf_t > 0
    selects the coarse tower features, prop_conf_t > 0 the refined ones; labels <= 0 are ignored;
  * per class and stage, MAV = class_means of its rows and the own-class distances come from the labelled wide distance
    kernel (otal_openmax_dist_wide);
  * files: <output_path>/openmax/mav_dist/<class name>.npz with the keys mav, dist, mav_prop, dist_prop (the layout of the
    THUMOS14 files).  A class without a positive in either stage raises the ValueError of common.openmax.save_mav_dist.  If the
    files are all there the pass is skipped; if they are missing and WORLD_SIZE > 1 the driver raises: the pass reads the
    whole training set once and is to be run once, in one process, before a multi-rank test.

Fits.  common.openmax.weibull_fitting with tailsize 20; two anet.openmax.OpenMax layers of rank 1.

Test pass.  The validation videos as anet.test.main selects them; each rank takes every world-th video;
common/detect.py's `detect` with the wide decode launch (otal_decode_clips_openmax_wide, get_feat=True) and ONE Soft-NMS
launch over 150 classes; get_video_prediction clips to the duration; gather_results to rank 0.  `--refined_feature` feeds
the refined feature to the refined stage's layer (thumos14/test_openmax.py explains the switch).

Result file.  <output_path>/openmax/<output_json> -- NOT the Softmax baseline's own file in <output_path>, which anet.test
would otherwise re-use as complete -- as {"version": "ActivityNet-v1.3", "results": ..., "external_data": {}}, written
through driver.write_json; 'uncertainty' and 'actionness' are 0.0, as for the Softmax baseline.  It evaluates with
`python -m opental_amd.anet.eval_open --open_set --ood_scoring confidence`.
"""
import functools
import json
import os
import sys

import torch

from ..common import detect as _d
from ..common import openmax as _common
from ..common.detect import prepare_data
from ..common.openmax import files_are_ready, save_mav_dist, weibull_fitting
from . import test as T
from .openmax import OpenMax

TAILSIZE = 20
mav_and_dist = functools.partial(_common.mav_and_dist, family=OpenMax.FAMILY)


def positive_labels(criterion, loc, priors, targets):
    """The anchors the training loss calls positive, by the loss's own matching: (conf_t, prop_conf_t) (B, A) long, 0 where
    an anchor has no ground truth (coarse) / its coarse segment misses the tIoU bar (refined)."""
    _, conf_t, _, prop_conf_t, _ = criterion.match(loc, priors, targets)
    return conf_t, prop_conf_t


@torch.no_grad()
def collect_features(net, criterion, samples, npy_path, clip_length=T.CLIP_LENGTH, crop_size=96, batch_clips=4, device='cuda'):
    """The statistics pass's loop over `samples` (split_videos records): the tower features and 0-based class indices of
    the positive anchors of both stages -> (feat (N, D), labels (N,) int32, prop_feat, prop_labels)."""
    from ..common.anet_dataset import annos_transform
    rows = []
    batch_clips = _d.windows_per_pass(batch_clips)
    for i in range(0, len(samples), batch_clips):
        part = samples[i:i + batch_clips]
        vids = [prepare_data(npy_path, s['video_name'], crop_size, device) for s in part]
        out = net(_d.prepare_windows(vids, [(v, 0) for v in range(len(part))], clip_length), get_feat=True)
        targets = [torch.tensor(annos_transform(s['annos'], clip_length), dtype=torch.float32).reshape(-1, 3) for s in part]
        conf_t, prop_conf_t = positive_labels(criterion, out['loc'], out['priors'], targets)
        rows.append(_common.positive_rows(out, conf_t, prop_conf_t))
    return _common.cat_rows(rows)


def compute_mav_dist(mav_dist_dir, net, idx_to_class, config, batch_clips=4, device='cuda'):
    """The statistics pass (module docstring) -> the mav_dist files."""
    from ..common.anet_dataset import get_video_info, split_videos
    from .multisegment_loss import MultiSegmentLoss
    tr = config['dataset']['training']
    samples, _ = split_videos(get_video_info(tr['video_info_path'], 'training'), tr['clip_length'], tr['video_mp4_path'])
    criterion = MultiSegmentLoss(config['dataset']['num_classes'], config['training']['piou'], 1.0, cls_loss_type='focal',
                                 os_head=False, clip_length=tr['clip_length']).to(device)
    K = len(idx_to_class)
    feat, lab, pfeat, plab = collect_features(net, criterion, samples, tr['video_mp4_path'], tr['clip_length'], tr['crop_size'],
                                              batch_clips, device)
    save_mav_dist(mav_dist_dir, idx_to_class, mav_and_dist(feat, lab, K) + (lab,), mav_and_dist(pfeat, plab, K) + (plab,))


def decode_clips_openmax(output_dict, fps, openmax_layer, openmax_prop_layer, clip_length=T.CLIP_LENGTH, conf_thresh=0.001,
                         refined_feature=False):
    """The batched decode of n videos (one clip each, offset 0) in one launch, otal_decode_clips_openmax_wide: both stages'
    recalibration, their average, the centre factor, the segments of anet/test.py:110-115 and flag = score > conf_thresh.
    output_dict: the closed-set network's outputs with get_feat=True (conf / prop_conf carry the background logit, which is
    dropped; the priors' level column is dropped too).  Returns dict(seg (n, A, 2), score (n, K, A), flag (n, K, A) uint8,
    unknown (n, A), unct None, actn None): the layout of decode_clips, so softnms_classes takes it as it is."""
    heads = T._heads(output_dict)
    return _common.decode_clips_openmax(heads, [0.0] * heads['loc'].shape[0], fps, openmax_layer, openmax_prop_layer,
                                        clip_length, conf_thresh, refined_feature)


def detect_rows(net, videos, sample_fps, openmax_layer, openmax_prop_layer, clip_length=T.CLIP_LENGTH, conf_thresh=0.001,
                top_k=5000, nms_sigma=0.85, batch_clips=4, refined_feature=False):
    """anet.test.detect_rows for the OpenMax baseline: the network with get_feat=True, the wide decode launch, one Soft-NMS
    launch; rows (V, K, min(top_k, A), 3) and counts (V, K) on the device."""
    if _d.head_mode(net)[0] or _d.head_mode(net)[1]:
        raise NotImplementedError("OpenMax runs on the closed-set Softmax network (model.os_head and model.use_edl false)")
    keys = ('loc', 'conf', 'prop_loc', 'prop_conf', 'center', 'conf_feat', 'prop_conf_feat', 'priors')
    decode = lambda merged, offsets, fps: decode_clips_openmax(merged, fps, openmax_layer, openmax_prop_layer, clip_length,
                                                               conf_thresh, refined_feature)
    return _d.detect(net, videos, sample_fps, decode, keys, clip_length, None, top_k, nms_sigma, batch_clips, get_feat=True)[:2]


def testing(net, video_list, video_infos, npy_path, openmax_layer, openmax_prop_layer, idx_to_class=None,
            clip_length=T.CLIP_LENGTH, crop_size=96, conf_thresh=0.001, top_k=5000, nms_sigma=0.85, batch_clips=4, rank=0,
            world=1, device='cuda', refined_feature=False):
    """anet.test.testing with the OpenMax decode: this rank's share (every world-th video) -> {name without "v_": proposals}."""
    mine = list(video_list)[rank::world]
    out = {}
    for i in range(0, len(mine), batch_clips):
        part = mine[i:i + batch_clips]
        vids = [prepare_data(npy_path, n, crop_size, device) for n in part]
        rows, counts = detect_rows(net, vids, [float(video_infos[n]['fps']) for n in part], openmax_layer, openmax_prop_layer,
                                   clip_length, conf_thresh, top_k, nms_sigma, batch_clips, refined_feature)
        for v, n in enumerate(part):
            out[n[2:]] = T.get_video_prediction(rows[v], counts[v], float(video_infos[n]['duration']), idx_to_class)
    return out


def main(argv=None):
    from ..common import config as C
    from ..common.driver import device_setup, load_net, split_flags, write_json
    from .BDNet import BDNet, model_cfg_from
    own, argv = split_flags(list(sys.argv[1:] if argv is None else argv), ('--random_init', '--refined_feature'))
    config = C.set_config(C.get_config(argv))
    te, md, ds = config['testing'], config['model'], config['dataset']
    t = ds['testing']
    if md.get('os_head', False) or md.get('use_edl', False):
        raise NotImplementedError("OpenMax runs on the closed-set Softmax network (model.os_head and model.use_edl false)")
    idx_to_class = T.get_class_names(ds['class_info_path'])
    out_dir = os.path.join(te['output_path'], 'openmax')
    mav_dist_dir = os.path.join(out_dir, 'mav_dist')
    ready = files_are_ready(mav_dist_dir, idx_to_class)
    if not ready and int(os.environ.get('WORLD_SIZE', 1)) > 1:
        raise RuntimeError(f"the mav_dist files under {mav_dist_dir} are missing: run the statistics pass once, in one process "
                           "(python -m opental_amd.anet.test_openmax without torchrun), before a multi-rank test")
    rank, world, dev = device_setup()
    net = load_net(BDNet, dev, own['--random_init'], te['checkpoint_path'], in_channels=md['in_channels'],
                   frame_num=t['clip_length'], use_edl=False, cfg=model_cfg_from(config))
    if not ready:
        compute_mav_dist(mav_dist_dir, net, idx_to_class, config, device=dev)
    weibull_model, weibull_prop_model = weibull_fitting(idx_to_class, mav_dist_dir, tailsize=TAILSIZE)
    layers = OpenMax(weibull_model, rank=1).to(dev), OpenMax(weibull_prop_model, rank=1).to(dev)
    with open(t['video_info_path']) as f:
        infos = {k: v for k, v in json.load(f).items() if v.get('subset', 'validation') == 'validation'}
    on_disk = {f[:-4] for f in os.listdir(t['video_mp4_path']) if f.endswith('.npy')}
    video_list = [n for n in infos if n in on_disk]
    res = testing(net, video_list, infos, t['video_mp4_path'], layers[0], layers[1], idx_to_class, t['clip_length'],
                  t['crop_size'], te['conf_thresh'], te['top_k'], te['nms_sigma'], rank=rank, world=world, device=dev,
                  refined_feature=own['--refined_feature'])
    res = _d.gather_results(res, [n[2:] for n in video_list], rank, world, dev)
    if res is None:
        return None
    assert len(res) == len(video_list), "Incomplete testing results!"
    out_file = os.path.join(out_dir, te['output_json'])
    write_json(out_file, _d.results_json(res, version="ActivityNet-v1.3"))
    print(f"{len(res)} videos, {sum(len(v) for v in res.values())} detections -> {out_file}")
    return out_file


if __name__ == '__main__':
    main()
