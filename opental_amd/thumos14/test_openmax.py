"""The OpenMax baseline's statistics pass and inference path on MI355X, with the reference's function names
(AFSD/thumos14/test_openmax.py): get_matched_targets (:102-138), compute_mav_dist (:248-327), weibull_fitting (:331-354),
decode_output (:141-170) as the batched decode_clips_openmax, test (:358-403) and the driver of :416-430.

OpenMax runs on the checkpoint of the closed-set Softmax baseline (configs/thumos14_openmax.yaml differs from
thumos14_softmax.yaml only in paths): no training.  The statistics pass sends every training clip through the eval-mode
network with get_feat=True, collects the 512-d tower features of the positive anchors per class and stage, and writes per
class <output_path>/mav_dist/<class name>.npz with the reference's keys (mav, dist, mav_prop, dist_prop), so the files are
interchangeable with the reference's.  Inference is detect_batch_openmax (common/detect.py's pipeline with the OpenMax
decode): the network, ONE OpenMax decode launch
(otal_decode_clips_openmax: both stages' recalibration, the average, the centre factor, segments and threshold flags) and ONE
Soft-NMS launch, with no host synchronisation before the final copy.  The reference instead loops on the host over every
anchor and class (openmax.py:76-86), twice per clip.

As shipped the reference feeds the COARSE feature to the refined stage's OpenMax layer too (test_openmax.py:159), although
that layer's MAVs were built from the refined features; `refined_feature=True` reads the refined feature instead.

decode_clips_openmax, mav_and_dist, save_mav_dist, files_are_ready and weibull_fitting are common/openmax.py's, shared with
the ActivityNet1.3 recipe and bound here under the reference's names.
"""
import functools
import os

import torch

from ..common import openmax as _common
from ..common.detect import detect, get_video_detections, head_mode, prepare_data, prepare_windows, results_json, windows_per_pass
from ..common.openmax import decode_clips_openmax, files_are_ready, save_mav_dist, weibull_fitting  # noqa: F401
from .openmax import OpenMax

mav_and_dist = functools.partial(_common.mav_and_dist, family=OpenMax.FAMILY)


def compute_iou(pred, target):
    """test_openmax.py:82-99 on (..., 2) tensors."""
    inter = torch.min(pred[..., 0], target[..., 0]) + torch.min(pred[..., 1], target[..., 1])
    union = (target[..., 0] + target[..., 1]) + (pred[..., 0] + pred[..., 1]) - inter
    return inter / union.clamp(min=torch.finfo(torch.float32).eps)


def get_matched_targets(targets, loc_data, priors, clip_length, tiou_thresh=0.5):
    """test_openmax.py:102-138, vectorised over the batch with torch ops on the device of `loc_data`.  targets: list of
    (G_b, 3) tensors [start, end, label] in clip units; loc_data (B, A, 2); priors (A, 1).  Returns loc_t (B, A, 2), conf_t
    (B, A) long, prop_loc_t, prop_conf_t: conf_t is the label of the enclosing ground truth with the smallest area (0
    without one), prop_conf_t the same zeroed where the tIoU of the coarse prediction is below `tiou_thresh`."""
    dev = loc_data.device
    B, A = loc_data.shape[0], priors.shape[0]
    G = max([int(t.shape[0]) for t in targets] + [1])
    gt = torch.zeros((B, G, 3), dtype=torch.float32)
    valid = torch.zeros((B, G), dtype=torch.bool)
    for b, t in enumerate(targets):
        n = int(t.shape[0])
        if n:
            gt[b, :n] = t.detach().to('cpu', torch.float32)
            valid[b, :n] = True
    gt, valid = gt.to(dev), valid.to(dev)
    center = priors[:, 0].to(dev).view(1, A, 1)
    left = (center - gt[:, :, 0].unsqueeze(1)) * clip_length            # (B, A, G)
    right = (gt[:, :, 1].unsqueeze(1) - center) * clip_length
    maxn = clip_length * 2
    area = left + right
    area = torch.where((left < 0) | (right < 0), torch.full_like(area, maxn), area)
    area = torch.where(valid.unsqueeze(1), area, torch.full_like(area, float('inf')))     # padding never wins
    best_area, best_idx = area.min(2)                                   # (B, A)
    t0 = torch.gather(gt[:, :, 0], 1, best_idx)
    t1 = torch.gather(gt[:, :, 1], 1, best_idx)
    loc_t = torch.stack([(center[..., 0] - t0) * clip_length, (t1 - center[..., 0]) * clip_length], -1)
    conf_t = torch.gather(gt[:, :, 2], 1, best_idx).long()
    conf_t = torch.where(best_area >= maxn, torch.zeros_like(conf_t), conf_t)
    iou = compute_iou(loc_data, loc_t)
    prop_conf_t = torch.where(iou < tiou_thresh, torch.zeros_like(conf_t), conf_t)
    prop_w = loc_data[..., 0] + loc_data[..., 1]
    prop_loc_t = (loc_t - loc_data) / (0.5 * prop_w).unsqueeze(-1)
    return loc_t, conf_t, prop_loc_t, prop_conf_t


def _train_video(data_path, name, crop_size, clip_length, device):
    """prepare_train_data (test_openmax.py:66-79): the centre-cropped planar uint8 video; one shorter than a clip is padded
    with ZERO frames before normalisation (they become -1.0, unlike the test path's padding with 0.0)."""
    data = prepare_data(data_path, name, crop_size, device)
    if data.shape[1] < clip_length:
        pad = torch.zeros((data.shape[0], clip_length - data.shape[1]) + tuple(data.shape[2:]), dtype=torch.uint8, device=device)
        data = torch.cat([data, pad], 1).contiguous()
    return data


@torch.no_grad()
def collect_features(net, samples, video_infos, data_path, clip_length, crop_size, tiou_thresh, batch_clips=32, device='cuda'):
    """The loop of compute_mav_dist (test_openmax.py:268-311), `batch_clips` training clips per forward pass: the features
    and 0-based class indices of the positive anchors of both stages -> (feat (N, D), labels (N,), prop_feat, prop_labels)."""
    from ..common.thumos_dataset import annos_transform
    rows = []
    batch_clips = windows_per_pass(batch_clips)
    order = sorted(range(len(samples)), key=lambda i: samples[i]['video_name'])       # one video on the device at a time
    cache = {}
    for i in range(0, len(order), batch_clips):
        part = [samples[j] for j in order[i:i + batch_clips]]
        names = sorted({s['video_name'] for s in part})
        cache = {n: cache[n] if n in cache else _train_video(data_path, n, crop_size, clip_length, device) for n in names}
        vids = [cache[n] for n in names]
        out = net(prepare_windows(vids, [(names.index(s['video_name']), int(s['offset'])) for s in part], clip_length),
                  get_feat=True)
        targets = [torch.tensor(annos_transform(s['annos'], clip_length), dtype=torch.float32).reshape(-1, 3) for s in part]
        _, conf_t, _, prop_conf_t = get_matched_targets(targets, out['loc'], out['priors'], clip_length, tiou_thresh)
        rows.append(_common.positive_rows(out, conf_t, prop_conf_t))
    return _common.cat_rows(rows)


def compute_mav_dist(mav_dist_dir, net, idx_to_class, video_infos, video_annos, data_path, clip_length=256, stride=30,
                     crop_size=96, tiou_thresh=0.5, batch_clips=32, device='cuda'):
    """test_openmax.py:248-327."""
    from ..common.thumos_dataset import split_videos
    data_list, _ = split_videos(video_infos, video_annos, clip_length=clip_length, stride=stride)
    K = len(idx_to_class)
    feat, lab, pfeat, plab = collect_features(net, data_list, video_infos, data_path, clip_length, crop_size, tiou_thresh,
                                              batch_clips, device)
    save_mav_dist(mav_dist_dir, idx_to_class, mav_and_dist(feat, lab, K) + (lab,), mav_and_dist(pfeat, plab, K) + (plab,))


def detect_batch_openmax(net, videos, sample_fps, openmax_layer, openmax_prop_layer, clip_length=256, stride=128,
                         conf_thresh=0.01, top_k=5000, nms_sigma=0.5, batch_clips=32, refined_feature=False):
    """detect_batch (thumos14/test.py) for the OpenMax baseline: every sliding window of `videos` through the network with
    get_feat=True, then the OpenMax decode launch and the Soft-NMS launch (common/detect.py's `detect`); nothing synchronises
    with the host before the caller copies the rows.  Returns (rows, counts, index, dec)."""
    if head_mode(net)[0]:
        raise NotImplementedError("OpenMax runs on the closed-set Softmax network (os_head false)")
    keys = ('loc', 'conf', 'prop_loc', 'prop_conf', 'center', 'conf_feat', 'prop_conf_feat', 'priors')
    decode = lambda merged, offsets, fps: decode_clips_openmax(merged, offsets, fps, openmax_layer, openmax_prop_layer,
                                                               clip_length, conf_thresh, refined_feature)
    return detect(net, videos, sample_fps, decode, keys, clip_length, stride, top_k, nms_sigma, batch_clips, get_feat=True)


def test(net, video_infos, npy_data_path, openmax_layer, openmax_prop_layer, idx_to_class=None, clip_length=256, stride=128,
         crop_size=96, conf_thresh=0.01, top_k=5000, nms_sigma=0.5, batch_clips=32, batch_videos=8, device='cuda',
         refined_feature=False):
    """The loop of test_openmax.py:358-399 over a video list, batched as thumos14/test.py's `test`."""
    names = list(video_infos.keys())
    result_dict = {}
    for i in range(0, len(names), batch_videos):
        part = names[i:i + batch_videos]
        vids = [prepare_data(npy_data_path, n, crop_size, device) for n in part]
        rows, counts, _, _ = detect_batch_openmax(net, vids, [float(video_infos[n]['sample_fps']) for n in part], openmax_layer,
                                                  openmax_prop_layer, clip_length, stride, conf_thresh, top_k, nms_sigma,
                                                  batch_clips, refined_feature)
        for v, n in enumerate(part):
            result_dict[n] = get_video_detections(rows[v], counts[v], idx_to_class, top_k)
    return result_dict


def main(argv=None):
    """python -m opental_amd.thumos14.test_openmax <yaml> --open_set --split N [--random_init] [--evaluate GT.json KNOWN.txt]

    The reference's driver (test_openmax.py:416-430): config -> the Softmax baseline's model + checkpoint -> the mav_dist
    files under <output_path>/mav_dist (computed from the training split unless they are all there) -> Weibull fits -> the
    two OpenMax layers (rank 1) -> sliding windows over every test video -> result JSON at <output_path>/<output_json>
    ('uncertainty' and 'actionness' 0.0, as for the Softmax baseline); `--evaluate` then runs the open-set evaluation with
    `ood_scoring: confidence`."""
    import sys
    from ..common import config as C
    from ..common.driver import device_setup, load_net, split_flags, write_json
    from ..common.thumos_dataset import get_class_index_map, get_video_anno, get_video_info
    from .BDNet import BDNet, model_cfg_from
    own, rest = split_flags(list(sys.argv[1:] if argv is None else argv), ('--random_init',), {'--evaluate': (2, None)})
    evaluate = own['--evaluate']
    config = C.set_config(C.get_config(rest))
    te, md, ds, dtr = config['testing'], config['model'], config['dataset']['testing'], config['dataset']['training']
    _, _, dev = device_setup()
    net = load_net(BDNet, dev, own['--random_init'], te['checkpoint_path'], in_channels=md['in_channels'],
                   use_edl=md.get('use_edl', False), cfg=model_cfg_from(config))
    if head_mode(net)[0] or head_mode(net)[1]:
        raise NotImplementedError("OpenMax runs on the closed-set Softmax network (model.os_head and model.use_edl false)")
    _, idx_to_class = get_class_index_map(config['dataset']['class_info_path'])
    mav_dist_dir = os.path.join(te['output_path'], 'mav_dist')
    if not files_are_ready(mav_dist_dir, idx_to_class):
        train_infos = get_video_info(dtr['video_info_path'])
        train_annos = get_video_anno(train_infos, dtr['video_anno_path'], config['dataset']['class_info_path'])
        compute_mav_dist(mav_dist_dir, net, idx_to_class, train_infos, train_annos, dtr['video_data_path'], dtr['clip_length'],
                         dtr['clip_stride'], dtr['crop_size'], config['training']['piou'], device=dev)
    weibull_model, weibull_prop_model = weibull_fitting(idx_to_class, mav_dist_dir)
    video_infos = get_video_info(ds['video_info_path'])
    results = test(net, video_infos, ds['video_data_path'], OpenMax(weibull_model), OpenMax(weibull_prop_model), idx_to_class,
                   ds['clip_length'], ds['clip_stride'], ds['crop_size'], te['conf_thresh'], te['top_k'], te['nms_sigma'],
                   device=dev)
    out_file = os.path.join(te['output_path'], te['output_json'])
    write_json(out_file, results_json(results))
    print(f"{len(results)} videos, {sum(len(v) for v in results.values())} detections -> {out_file}")
    if evaluate is not None:
        from .eval_open import evaluate_split
        return out_file, evaluate_split(out_file, evaluate[0], evaluate[1], [0.3, 0.4, 0.5, 0.6, 0.7], ['test'], True, 'confidence')
    return out_file, None


if __name__ == '__main__':
    main()
