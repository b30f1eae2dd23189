"""Inference path of OpenTAL/AFSD on MI355X for THUMOS14, with the reference's function names (AFSD/thumos14/test.py):
prepare_clip (:67-76), the RPL / GCPL flags of :268-269, test (:203-252) and the driver (:255-288).

`detect_batch` is the MI355X-first entry point: common/detect.py's `detect` (batched sliding windows, ONE decode launch, ONE
Soft-NMS launch, no host synchronisation until the final copy) with the decode the THUMOS14 head asks for (test.py:79-162):
the OpenTAL head (os_head + use_edl: Dirichlet scores x actionness; otal_decode_clips) and the closed-set Softmax / EDL
baselines (os_head false: softmax or Dirichlet scores over C = classes + 1 logits, the background class dropped, no
actionness; otal_decode_clips_ex).  Everything that does not depend on the dataset lives in common/detect.py and is
imported here under the names it has always had in this module.
"""
import torch

from ..common.detect import (OOD_SCORES, _decode_clips_ex, decode_clips, decode_clips_two_stream,  # noqa: F401
                             decode_predictions, detect, filtering, fuse_outputs, gather_results, get_offsets, get_video_detections, head_mode, ood_threshold,
                             prepare_data, prepare_windows, results_json, rpl_logits, softnms_classes)


def prepare_clip(data, offset, clip_length):
    """uint8 (C,T,H,W) device tensor -> (1,C,clip_length,H,W) float in [-1,1], zero padded (test.py:67-76)."""
    clip = data[:, offset: offset + clip_length].float()
    clip = (clip / 255.0) * 2.0 - 1.0
    if clip.size(1) < clip_length:
        pad = torch.zeros([clip.size(0), clip_length - clip.size(1), clip.size(2), clip.size(3)], device=clip.device)
        clip = torch.cat([clip, pad], dim=1)
    return clip.unsqueeze(0)


def rpl_flags(config):
    """(use_rpl, use_gcpl) of a parsed config, as test.py:268-269 reads them: the distance head of the RPL / GCPL baselines
    and whether its scores are the softmax of the NEGATED distances."""
    use_rpl = bool(config['model'].get('use_rpl', False))
    rc = config['training'].get('rpl_config') or {}
    return use_rpl, bool(use_rpl and rc.get('gcpl', False))


def detect_batch(net, videos, sample_fps, clip_length=256, stride=128, conf_thresh=0.01, top_k=5000, nms_sigma=0.5,
                 batch_clips=32, flow_net=None, flow_videos=None, two_stream_decode=True):
    """videos: list of uint8 (C,T,96,96) device tensors (already centre-cropped).  Returns the
    per-video rows/counts of Soft-NMS.  test.py:203-252 without the JSON dump.
    Two-stream runs (`--fusion`, test.py:227-240 + parse_output :90-108): `flow_net` sees the same windows of
    `flow_videos` (2-channel optical flow) and the two networks' RAW outputs are averaged before decoding -- inside the decode
    launch (decode_clips_two_stream: the raw maps of both networks go in, no averaged copy is written).
    two_stream_decode=False: the earlier route with the same results (torch.equal rows, counts, index and dec) -- fuse_outputs
    per chunk of windows, decode_clips on the averaged maps, the uncertainty substituted afterwards."""
    if (flow_net is None) != (flow_videos is None):
        raise RuntimeError("detect_batch: flow_net and flow_videos go together")
    os_head, use_edl, evidence = head_mode(net)
    if flow_net is not None and head_mode(flow_net) != (os_head, use_edl, evidence):
        raise RuntimeError(f"detect_batch: the rgb and flow networks have different heads "
                           f"({(os_head, use_edl, evidence)} vs {head_mode(flow_net)})")
    keys = ('loc', 'conf', 'prop_loc', 'prop_conf', 'center', 'priors') + (('act', 'prop_act') if os_head else ()) + \
        (('unct', 'prop_unct') if flow_net is not None and use_edl else ())

    use_gcpl = bool(getattr(net, 'use_gcpl', False))

    def decode(merged, offsets, fps):
        dec = decode_clips(merged, offsets, fps, clip_length, conf_thresh, os_head=os_head, use_edl=use_edl,
                           evidence=evidence, use_gcpl=use_gcpl)
        if flow_net is not None and use_edl:
            # the decode kernel derives the uncertainty from the (fused) logits; the reference averages the two networks'
            # OWN uncertainties instead (parse_output :105-108, decode_predictions :122) -- not the same number
            dec['unct'] = ((merged['unct'] + merged['prop_unct']) / 2.0).contiguous()
        return dec

    def decode_two_stream(rgb, flow, offsets, fps):         # the same, from the two networks' raw maps in one launch
        return decode_clips_two_stream(rgb, flow, offsets, fps, clip_length, conf_thresh, os_head=os_head, use_edl=use_edl,
                                       evidence=evidence, use_gcpl=use_gcpl)
    return detect(net, videos, sample_fps, decode, keys, clip_length, stride, top_k, nms_sigma, batch_clips, flow_net,
                  flow_videos, decode_two_stream, two_stream_decode)


def test(net, video_infos, npy_data_path, idx_to_class=None, clip_length=256, stride=128, crop_size=96, conf_thresh=0.01,
         top_k=5000, nms_sigma=0.5, batch_clips=32, batch_videos=8, rank=0, world=1, device='cuda', flow_net=None,
         flow_data_path=None):
    """The loop of test.py:203-252 over a video list, batched: `batch_videos` videos' windows go through the network
    together and ONE decode + ONE Soft-NMS launch serve all of them.  Ranks take every world-th video (no collective).
    `flow_net` + `flow_data_path`: the two-stream (fusion) run of test.py:213-240."""
    names = list(video_infos.keys())[rank::world]
    result_dict = {}
    for i in range(0, len(names), batch_videos):
        part = names[i:i + batch_videos]
        vids = [prepare_data(npy_data_path, n, crop_size, device) for n in part]
        flows = [prepare_data(flow_data_path, n, crop_size, device) for n in part] if flow_net is not None else None
        rows, counts, _, _ = detect_batch(net, vids, [float(video_infos[n]['sample_fps']) for n in part], clip_length, stride,
                                          conf_thresh, top_k, nms_sigma, batch_clips, flow_net=flow_net, flow_videos=flows)
        for v, n in enumerate(part):
            result_dict[n] = get_video_detections(rows[v], counts[v], idx_to_class, top_k)
    return result_dict


def main(argv=None):
    """python -m opental_amd.thumos14.test <yaml> --open_set --split 0 [--random_init] [--evaluate GT.json KNOWN.txt]

    The reference's test driver (AFSD/thumos14/test.py:203-288): config -> model + checkpoint -> sliding windows over
    every test video -> result JSON at <output_path>/<output_json>; `--evaluate` then runs the open-set evaluation of
    opental_amd.thumos14.eval_open on it."""
    import os
    import sys
    from ..common import config as C
    from ..common.driver import device_setup, load_net, split_flags, write_json
    from ..common.thumos_dataset import get_class_index_map, get_video_info
    from .BDNet import BDNet, model_cfg_from
    own, rest = split_flags(list(sys.argv[1:] if argv is None else argv), ('--random_init',), {'--evaluate': (2, None)})
    random_init, evaluate = own['--random_init'], own['--evaluate']
    config = C.set_config(C.get_config(rest))
    te, md, ds = config['testing'], config['model'], config['dataset']['testing']
    rank, world, dev = device_setup()
    flow_net, data_path, flow_path = None, ds['video_data_path'], None
    use_rpl, use_gcpl = rpl_flags(config)
    kw = dict(use_edl=md.get('use_edl', False), use_rpl=use_rpl, cfg=model_cfg_from(config))
    if te.get('fusion', False):             # build_model(fusion=True), test.py:24-40: rgb + flow networks, their own checkpoints
        net = load_net(BDNet, dev, random_init, te.get('rgb_checkpoint_path', './models/thumos14/checkpoint-15.ckpt'),
                       in_channels=3, **kw)
        flow_net = load_net(BDNet, dev, random_init, te.get('flow_checkpoint_path', './models/thumos14_flow/checkpoint-16.ckpt'),
                            in_channels=2, **kw)
        data_path = te.get('rgb_data_path', './datasets/thumos14/test_npy/')
        flow_path = te.get('flow_data_path', './datasets/thumos14/test_flow_npy/')
    else:
        net = load_net(BDNet, dev, random_init, te['checkpoint_path'], in_channels=md['in_channels'], **kw)
    net.use_gcpl = use_gcpl                 # GCPL: scores are the softmax of the negated distances (detect_batch)
    video_infos = get_video_info(config['dataset']['testing']['video_info_path'])
    _, idx_to_class = get_class_index_map(config['dataset']['class_info_path'])
    results = test(net, video_infos, data_path, idx_to_class, ds['clip_length'], ds['clip_stride'], ds['crop_size'],
                   te['conf_thresh'], te['top_k'], te['nms_sigma'], rank=rank, world=world, device=dev, flow_net=flow_net,
                   flow_data_path=flow_path)
    results = gather_results(results, list(video_infos.keys()), rank, world, dev)
    if results is None:
        return None, None           # ranks > 0: their detections went to rank 0
    out_file = os.path.join(te['output_path'], te['output_json'])
    write_json(out_file, results_json(results))
    print(f"{len(results)} videos, {sum(len(v) for v in results.values())} detections -> {out_file}")
    if evaluate is not None:
        from .eval_open import evaluate_split
        return out_file, evaluate_split(out_file, evaluate[0], evaluate[1], [0.3, 0.4, 0.5, 0.6, 0.7], ['test'], True,
                                        te.get('ood_scoring', 'confidence'))
    return out_file, None


if __name__ == '__main__':
    main()
