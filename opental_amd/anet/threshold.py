"""python -m opental_amd.anet.threshold configs/anet_opental.yaml --open_set --split 0 --ood_scoring uncertainty \\
       --output_json threshold_results.json [--random_init] [--keep_detections]

The known / unknown operating point of the ActivityNet1.3 open-set evaluation (AFSD/anet/threshold.py): the detector runs
over the TRAINING videos, every detection becomes a known-ness score (1 - its out-of-distribution score under
`--ood_scoring`) and the threshold is the value 95 % of them exceed (compute_threshold, :13-28, pinned in
tests/golden/anet_threshold.npz).  The file written is {"version": "ActivityNet-v1.3", "results": {...},
"external_data": {"threshold": t}}; an existing file that carries a threshold is re-used and printed, before any GPU
initialisation.

The reference's script does not run as shipped (it hands inference_thread six arguments for five), so the behaviour is
defined here on the model of thumos14/threshold.py, with these decisions:
  * videos: the `training` subset of dataset.training.video_info_path whose .npy exists in
    dataset.training.video_mp4_path, in file order.  The reference intersects the list with result_tsn_train.json, the
    video-level classifier's output that AFSD fuses into its ActivityNet results; nothing here reads such a file, the
    intersection is an AFSD leftover and is dropped;
  * no dicts: per batch the network, the decode launch and the Soft-NMS launch (anet.test.detect_rows) are followed by
    otal_detection_table (common/det_table.py), whose known-ness column is kept on the device; the threshold is one sort of
    that column.  The reference's `results` (one dict per detection of ~10 k videos, a multi-gigabyte file nobody reads --
    the evaluation consumes external_data.threshold only) is {} unless --keep_detections asks for it;
  * ranks of a torchrun launch take every world-th video as anet.test does; their score arrays are gathered on rank 0.
One host synchronisation per batch: the number of valid rows, to cut the score column to size."""
import json
import os
import sys

import torch

from ..common.det_table import detection_table, proposals_from_table, threshold_from_scores
from ..common.detect import gather_results, results_json
from ..common.driver import device_setup, load_net, split_flags, write_json
from . import test as T


def select_videos(video_info_path, npy_path):
    """-> (names, infos): the `training` videos of the info file that exist as <npy_path>/<name>.npy, in file order."""
    with open(video_info_path) as f:
        infos = {k: v for k, v in json.load(f).items() if v.get('subset') == 'training'}
    on_disk = {f[:-4] for f in os.listdir(npy_path) if f.endswith('.npy')}
    return [n for n in infos if n in on_disk], infos


def known_scores(detect, video_list, video_infos, scoring='uncertainty', batch_videos=8, rank=0, world=1, keep=False,
                 idx_to_class=None):
    """This rank's share of the pass.  detect(names) -> the Soft-NMS rows (V,K,top_k,cols) and counts (V,K) of these videos.
    Returns (the known-ness scores of every detection, fp64 on the rows' device; {name without "v_": proposal list}, filled
    only with `keep`)."""
    mine = list(video_list)[rank::world]
    parts, results = [], {}
    for i in range(0, len(mine), batch_videos):
        part = mine[i:i + batch_videos]
        rows, counts = detect(part)
        table = detection_table(rows, counts, [float(video_infos[n]['duration']) for n in part], scoring=scoring)
        parts.append(table['known'][:int(table['n'])].clone())
        if keep:
            results.update(proposals_from_table(table, [n[2:] for n in part], idx_to_class))
    return merge_scores(parts), results


def merge_scores(parts):
    """The score arrays of several batches or ranks as one fp64 column (the threshold does not depend on their order)."""
    parts = [torch.as_tensor(p, dtype=torch.float64).reshape(-1) for p in parts]
    return torch.cat(parts) if parts else torch.zeros(0, dtype=torch.float64)


def gather_scores(scores, rank, world, device=None):
    """Several ranks: every rank's score column travels to rank 0, which returns them merged in rank order; the other ranks
    return None.  One rank: the column itself."""
    if world == 1:
        return scores
    parts = gather_results({rank: scores.cpu().numpy()}, list(range(world)), rank, world, device)
    return None if parts is None else merge_scores(list(parts.values()))


def write_threshold_file(output_file, threshold, results=None):
    """The file of this pass: the threshold, and the detections when they were kept (driver.write_json: the re-use test of
    `main` never sees half a file)."""
    write_json(output_file, results_json(results or {}, threshold=threshold, version="ActivityNet-v1.3"))


def read_threshold_file(output_file):
    """The threshold of an existing file, or None."""
    if not os.path.exists(output_file):
        return None
    with open(output_file) as f:
        return json.load(f).get('external_data', {}).get('threshold')


def thresholding(net, video_list, video_infos, npy_path, output_file, idx_to_class=None, scoring='uncertainty',
                 clip_length=T.CLIP_LENGTH, crop_size=96, conf_thresh=0.001, top_k=5000, nms_sigma=0.85, batch_videos=8,
                 batch_clips=4, rank=0, world=1, device='cuda', keep_detections=False):
    """The pass over `video_list` and the file.  Returns the threshold on rank 0 (None on the other ranks)."""
    def detect(names):
        vids = [T.prepare_data(npy_path, n, crop_size, device) for n in names]
        fps = [float(video_infos[n]['fps']) for n in names]
        return T.detect_rows(net, vids, fps, clip_length, conf_thresh, top_k, nms_sigma, batch_clips)
    scores, results = known_scores(detect, video_list, video_infos, scoring, batch_videos, rank, world, keep_detections,
                                   idx_to_class)
    scores = gather_scores(scores, rank, world, device)
    if keep_detections:
        results = gather_results(results, [n[2:] for n in video_list], rank, world, device)
    if scores is None:
        return None
    thr = threshold_from_scores(scores)
    write_threshold_file(output_file, thr, results if keep_detections else None)
    return thr


def main(argv=None):
    from ..common import config as C
    own, argv = split_flags(list(sys.argv[1:] if argv is None else argv), ('--random_init', '--keep_detections'))
    args = C.build_parser().parse_args(argv)
    config = C.set_config(C.get_config(argv))
    te, md, ds = config['testing'], config['model'], config['dataset']
    output_file = os.path.join(te['output_path'], te['output_json'])
    thr = read_threshold_file(output_file)
    if thr is not None:
        print(f'Thresholding result file already exist at {output_file}!')
        print(f'The threshold is: {thr:.12f}')
        return output_file, thr
    from .BDNet import BDNet, model_cfg_from
    rank, world, dev = device_setup()
    tr, t = ds['training'], ds['testing']
    net = load_net(BDNet, dev, own['--random_init'], te['checkpoint_path'], in_channels=md['in_channels'],
                   frame_num=t['clip_length'], use_edl=md.get('use_edl', False), cfg=model_cfg_from(config))
    video_list, infos = select_videos(tr['video_info_path'], tr['video_mp4_path'])
    idx_to_class = None
    if ds.get('class_info_path') and os.path.exists(ds['class_info_path']):
        idx_to_class = T.get_class_names(ds['class_info_path'])
    thr = thresholding(net, video_list, infos, tr['video_mp4_path'], output_file, idx_to_class, args.ood_scoring,
                       t['clip_length'], t['crop_size'], te['conf_thresh'], te['top_k'], te['nms_sigma'], rank=rank,
                       world=world, device=dev, keep_detections=own['--keep_detections'])
    if thr is not None:
        print(f'{len(video_list)} training videos -> {output_file}')
        print(f'The threshold is: {thr:.12f}')
    return output_file, thr


if __name__ == '__main__':
    main()
