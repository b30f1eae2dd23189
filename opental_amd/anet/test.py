"""Inference path of the ActivityNet1.3 recipe on MI355X, with the reference's function names (AFSD/anet/test.py):
prepare_clip (:83-92), decode_prediction (:95-132), filtering (:135-156), get_video_prediction (:159-200).

A video is ONE 768-frame clip here (the data is resampled to the clip length, anet/test.py:71-80), so a batch of videos
is a batch of clips: the network runs on them together and the same two launches as THUMOS14 finish the job --
otal_decode_clips (refine + decode + Dirichlet scores + thresholds, for every clip; otal_decode_clips_ex for the closed-set
Softmax and EDL heads) and otal_softnms_classes (one workgroup per (video, class)).  Differences from the THUMOS14 file
that are kept: short videos are padded with 127.5 (mid-grey), the confidence threshold is 0.001, proposals are clipped to
[0, duration] and empty ones dropped.  The pipeline itself is common/detect.py's (one window per video), shared with
THUMOS14.  `detect_rows` ends after the two launches, with the Soft-NMS rows on the device
(anet/threshold.py turns them into a table there); `detect_batch` adds the host loop that builds the proposal dicts.
"""
import torch

from ..common import detect as _d
from ..common.detect import prepare_data                   # anet/test.py:71-80 reads the .npy as thumos14/test.py does

CLIP_LENGTH = 768


def prepare_clip(data, offset, clip_length=CLIP_LENGTH, crop_size=96):
    """uint8 (C,T,H,W) device tensor -> (1,C,clip_length,H,W) float in [-1,1]; the tail is padded with 127.5 -> 0.0."""
    clip = data[:, offset: offset + clip_length].float()
    if clip.size(1) < clip_length:
        pad = torch.full([clip.size(0), clip_length - clip.size(1), crop_size, crop_size], 127.5, device=clip.device)
        clip = torch.cat([clip, pad], dim=1)
    return ((clip / 255.0) * 2.0 - 1.0).unsqueeze(0)


def _heads(output_dict):
    """The ActivityNet priors carry the level id in a second column (anet/BDNet.py:262-269); decoding uses the centres."""
    d = dict(output_dict)
    if d['priors'].dim() == 2 and d['priors'].shape[1] > 1:
        d['priors'] = d['priors'][:, 0].contiguous()
    return d


def decode_clips(output_dict, fps, clip_length=CLIP_LENGTH, conf_thresh=0.001, os_head=True, use_edl=True, evidence='exp'):
    """Batched decode_prediction + the threshold masks of filtering for n videos (offset 0).  os_head / use_edl / evidence:
    the network's head (common.detect.head_mode).  The closed-set heads (os_head False: anet_softmax.yaml with softmax
    scores, anet_edl.yaml with Dirichlet scores) leave the background logit out of score / flag, so row c is the
    reference's class c + 1, and apply no actionness factor or mask (anet/test.py:95-156 with os_head False)."""
    n = output_dict['loc'].shape[0]
    return _d.decode_clips(_heads(output_dict), [0.0] * n, fps, clip_length, conf_thresh, os_head=os_head,
                           use_edl=use_edl, evidence=evidence)


def decode_prediction(output_dict, idx=0, sample_fps=1.0, clip_length=CLIP_LENGTH, os_head=True, use_edl=True, evidence='exp'):
    """Single-clip view: decoded_segments (A,2) in SECONDS (the reference divides by fps in filtering), conf_scores
    (K,A), uncertainty (A,) or None without use_edl, actionness (A,) or None without os_head."""
    return _d.decode_predictions(_heads(output_dict), idx, 0.0, sample_fps, clip_length, os_head=os_head, use_edl=use_edl,
                                 evidence=evidence)


def filtering(decoded_segments, conf_score_cls, uncertainty, actionness, conf_thresh=0.001, use_edl=True, os_head=True):
    return _d.filtering(decoded_segments, conf_score_cls, uncertainty, actionness, conf_thresh, use_edl=use_edl,
                        os_head=os_head)


def get_video_prediction(rows, counts, duration, idx_to_class=None):
    """anet/test.py:159-200: the proposal list of one video from its suppressed rows (K,top_k,cols), clipped to
    [0, duration]; proposals that end before they start are dropped."""
    return _d.get_video_detections(rows, counts, idx_to_class, duration=duration)


def detect_rows(net, videos, sample_fps, clip_length=CLIP_LENGTH, conf_thresh=0.001, top_k=5000, nms_sigma=0.85, batch_clips=4):
    """videos: list of uint8 (C,T,96,96) device tensors (centre-cropped).  Returns the Soft-NMS output of the batch, rows
    (V,K,min(top_k,A),cols) and counts (V,K), on the device: the network, one decode launch, one Soft-NMS launch
    (common/detect.py's `detect` with one window per video).  The network's head (os_head, use_edl, evidence) picks the
    decode.  The windows hold the same values as prepare_clip per video (127.5 padded before the normalisation IS 0.0)."""
    os_head, use_edl, evidence = _d.head_mode(net)
    keys = ('loc', 'conf', 'prop_loc', 'prop_conf', 'center', 'priors') + (('act', 'prop_act') if os_head else ())
    decode = lambda merged, offsets, fps: decode_clips(merged, fps, clip_length, conf_thresh, os_head=os_head,
                                                       use_edl=use_edl, evidence=evidence)
    return _d.detect(net, videos, sample_fps, decode, keys, clip_length, None, top_k, nms_sigma, batch_clips)[:2]


def detect_batch(net, videos, sample_fps, durations, idx_to_class=None, clip_length=CLIP_LENGTH, conf_thresh=0.001,
                 top_k=5000, nms_sigma=0.85, batch_clips=4):
    """detect_rows, then the host loop: returns {index: proposal list} clipped to the videos' durations."""
    rows, counts = detect_rows(net, videos, sample_fps, clip_length, conf_thresh, top_k, nms_sigma, batch_clips)
    return {v: get_video_prediction(rows[v], counts[v], durations[v], idx_to_class) for v in range(len(videos))}


# ----------------------------------------------------------------------------- the driver (anet/test.py:203-348)
def get_class_names(class_info_path):
    """anet/test.py:54-59: one class name per line -> {1..K: name}."""
    with open(class_info_path) as f:
        return {i + 1: line.strip() for i, line in enumerate(f.readlines())}


def testing(net, video_list, video_infos, npy_path, idx_to_class=None, clip_length=CLIP_LENGTH, crop_size=96, conf_thresh=0.001,
            top_k=5000, nms_sigma=0.85, batch_clips=4, rank=0, world=1, device='cuda'):
    """anet/test.py:294-331 over this rank's share of the video list (every world-th video: the reference's
    testing_multithread :248-273 splits the list over mp.Process workers; here the workers are the ranks of a torchrun
    launch, one per GPU, and the per-rank dicts are gathered on rank 0).  Returns {name without "v_": proposal list}."""
    mine = list(video_list)[rank::world]
    out = {}
    for i in range(0, len(mine), batch_clips):
        part = mine[i:i + batch_clips]
        vids = [prepare_data(npy_path, n, crop_size, device) for n in part]
        fps = [float(video_infos[n]['fps']) for n in part]                # sample_fps = video_infos[name]['fps'] (:74)
        res = detect_batch(net, vids, fps, [float(video_infos[n]['duration']) for n in part], idx_to_class, clip_length,
                           conf_thresh, top_k, nms_sigma, batch_clips)
        for v, n in enumerate(part):
            out[n[2:]] = res[v]
    return out


def main(argv=None):
    """python -m opental_amd.anet.test configs/anet_opental.yaml --open_set --split 0 [--random_init]

    anet/test.py:334-348: the validation videos that exist on disk, a complete result file re-used, else the run; the file is
    {"version": "ActivityNet-v1.3", "results": {...}, "external_data": {}} at <output_path>/<output_json>."""
    import json
    import os
    import sys
    from ..common import config as C
    from ..common.driver import device_setup, load_net, split_flags, write_json
    from .BDNet import BDNet, model_cfg_from
    own, argv = split_flags(list(sys.argv[1:] if argv is None else argv), ('--random_init',))
    config = C.set_config(C.get_config(argv))
    te, md, ds = config['testing'], config['model'], config['dataset']
    t = ds['testing']
    with open(t['video_info_path']) as f:
        infos = {k: v for k, v in json.load(f).items() if v.get('subset', 'validation') == 'validation'}
    on_disk = {f[:-4] for f in os.listdir(t['video_mp4_path']) if f.endswith('.npy')}
    video_list = [n for n in infos if n in on_disk]
    out_file = os.path.join(te['output_path'], te['output_json'])
    if os.path.exists(out_file):
        with open(out_file) as f:
            if len(json.load(f)['results']) == len(video_list):
                print(f'Result file exist and it is complete! \n{out_file}')
                return out_file
    rank, world, dev = device_setup()
    net = load_net(BDNet, dev, own['--random_init'], te['checkpoint_path'], in_channels=md['in_channels'],
                   frame_num=t['clip_length'], use_edl=md.get('use_edl', False), cfg=model_cfg_from(config))
    idx_to_class = None
    if ds.get('class_info_path') and os.path.exists(ds['class_info_path']):
        idx_to_class = get_class_names(ds['class_info_path'])
    res = testing(net, video_list, infos, t['video_mp4_path'], idx_to_class, t['clip_length'], t['crop_size'], te['conf_thresh'],
                  te['top_k'], te['nms_sigma'], rank=rank, world=world, device=dev)
    res = _d.gather_results(res, [n[2:] for n in video_list], rank, world, dev)
    if res is None:
        return None
    assert len(res) == len(video_list), "Incomplete testing results!"
    write_json(out_file, _d.results_json(res, version="ActivityNet-v1.3"))
    print(f"{len(res)} videos, {sum(len(v) for v in res.values())} detections -> {out_file}")
    return out_file


if __name__ == '__main__':
    main()
