"""python -m opental_amd.thumos14.analyze_anchors <yaml> --open_set --split N --subset test|train --target T
       [--all_windows] [--keep_rows] --output_npz F [--plots DIR] [--random_init]

The reference's diagnosis of a trained detector at the anchors, before decoding and Soft-NMS: the score distributions of
experiments/analyze_actionness.py and AFSD/thumos14/draw_distribution.py (known / unknown / background, per stage) and the
EDL gradient density of experiments/analyze_gradnorm.py, from ONE pass over the windows.  The reference saves every head
output of every window to an .npz and loops over it in numpy and torch-CPU; here the windows go through the network in
chunks (common/detect.py), each batch of windows is ONE otal_anchor_stats launch (the rule: common/anchor_stats.py), the
histograms stay on the device and are copied once at the end.

Windows (get_all_annos, analyze_actionness.py:160-203): the sliding windows at the test stride; a window is kept when some
annotation lies wholly inside it, with the annotations of ioa >= 0.5 clipped to it.  Labels come from the full class list
(Class_Index_All.txt next to the split's known list), so the held-out classes are above n_known.  `--all_windows` adds the
other windows with no ground truth: all their anchors are background (draw_distribution.py:357-369).

The .npz holds hist_score (2 stages, 3 groups, bins), hist_grad (2, bins), their edges, the per-group counts and the config
that matters (target, piou, bins, split, subset); with `--keep_rows` also label / value / grad (windows, K, 2) and the windows'
videos and offsets.  `--plots DIR` draws the reference's figures as step histograms (no KDE curves: seaborn is not needed).

THUMOS14 only: the ActivityNet recipe matches differently and the reference has no such tool for it."""
import os
import sys

import numpy as np
import torch

from ..common.anchor_stats import GROUPS, STAGES, anchor_stats, check_mode, grad_edges, score_edges
from ..common.detect import forward_windows, get_offsets, head_mode, prepare_data
from ..common.driver import device_setup, load_net, split_flags


def select_windows(video_infos, video_annos, clip_length=256, stride=128, all_windows=False):
    """get_all_annos (analyze_actionness.py:160-203) without its start / end maps: [{'video_name', 'offset', 'annos'}] in the
    order of `video_annos`, annos = [[start, end, label]] in frames of the window.  all_windows: every window of every
    annotated video, the ones get_all_annos drops with annos = []."""
    out = []
    for name, annos in video_annos.items():
        for offset in get_offsets(video_infos[name]['sample_count'], clip_length, stride):
            left, right = offset + 1, offset + clip_length
            cur, keep = [], False
            for a in annos:
                ioa = (min(right, a[1]) - max(left, a[0])) * 1.0 / (a[1] - a[0])
                if ioa >= 1.0:
                    keep = True
                if ioa >= 0.5:
                    cur.append([max(a[0] - offset, 1), min(a[1] - offset, clip_length), a[2]])
            if keep:
                out.append({'video_name': name, 'offset': offset, 'annos': cur})
            elif all_windows:
                out.append({'video_name': name, 'offset': offset, 'annos': []})
    return out


def pad_targets(annos_per_window, clip_length, device):
    """annos_transform + padding: gt (B, G, 3) float32 in units of the clip, gvalid (B, G) uint8; G >= 1."""
    G = max(1, max(len(a) for a in annos_per_window))
    gt = np.zeros((len(annos_per_window), G, 3), np.float32)
    gvalid = np.zeros((len(annos_per_window), G), np.uint8)
    for b, annos in enumerate(annos_per_window):
        for g, a in enumerate(annos):
            gt[b, g] = (a[0] * 1.0 / clip_length, a[1] * 1.0 / clip_length, a[2])
            gvalid[b, g] = 1
    return torch.from_numpy(gt).to(device), torch.from_numpy(gvalid).to(device)


def head_keys(os_head):
    return ('loc', 'conf', 'prop_conf', 'center', 'priors') + (('act', 'prop_act') if os_head else ())


@torch.no_grad()
def analyze(net, windows, npy_data_path, target, overlap_thresh, n_known, clip_length=256, crop_size=96, score_bins=100,
            grad_bins=100, batch_videos=8, batch_clips=32, keep_rows=False, device='cuda'):
    """The statistics of `windows` (select_windows) -> dict of host arrays: hist_score, hist_grad, and with keep_rows label,
    value, grad (len(windows), K, 2) in the windows' order.  The windows of `batch_videos` videos form one batch: their
    forward passes in chunks of `batch_clips`, then one otal_anchor_stats launch."""
    os_head, use_edl, evidence = head_mode(net)
    check_mode(target, os_head, use_edl)
    names = list(dict.fromkeys(w['video_name'] for w in windows))
    hists = dict(hist_score=torch.zeros((2, 3, score_bins), dtype=torch.int64, device=device),
                 hist_grad=torch.zeros((2, grad_bins), dtype=torch.int64, device=device))
    rows = {k: [] for k in ('label', 'value', 'grad')}
    order = []
    for i in range(0, len(names), batch_videos):
        part = names[i:i + batch_videos]
        videos = [prepare_data(npy_data_path, n, crop_size, device) for n in part]
        idx = [j for j, w in enumerate(windows) if w['video_name'] in part]
        clips = [(part.index(windows[j]['video_name']), windows[j]['offset']) for j in idx]
        heads = forward_windows(net, videos, clips, clip_length, batch_clips, head_keys(os_head))
        gt, gvalid = pad_targets([windows[j]['annos'] for j in idx], clip_length, device)
        res = anchor_stats(heads['loc'], heads['conf'], heads['prop_conf'], heads['center'], heads.get('act'),
                           heads.get('prop_act'), heads['priors'], gt, gvalid, clip_length, overlap_thresh, os_head, n_known,
                           target, score_bins, grad_bins, out=hists, rows=keep_rows, evidence=evidence)
        if keep_rows:
            for k in rows:
                rows[k].append(res[k])
            order += idx
    out = {k: v.cpu().numpy() for k, v in hists.items()}
    if keep_rows:
        inv = np.argsort(np.array(order, dtype=np.int64))
        out.update({k: torch.cat(v, 0).cpu().numpy()[inv] for k, v in rows.items()})
    return out


def npz_payload(stats, windows, target, overlap_thresh, split, subset, n_known):
    score_bins, grad_bins = stats['hist_score'].shape[-1], stats['hist_grad'].shape[-1]
    out = dict(stats, score_edges=score_edges(score_bins), grad_edges=grad_edges(grad_bins).astype(np.float64),
               group_counts=stats['hist_score'].sum(-1), stages=np.array(STAGES), groups=np.array(GROUPS),
               target=np.array(target), piou=np.array(float(overlap_thresh)), score_bins=np.array(score_bins),
               grad_bins=np.array(grad_bins), split=np.array(int(split)), subset=np.array(subset), n_known=np.array(int(n_known)),
               n_windows=np.array(len(windows)))
    if 'label' in stats:
        out.update(window_video=np.array([w['video_name'] for w in windows]),
                   window_offset=np.array([w['offset'] for w in windows], dtype=np.int64))
    return out


def grad_weights(counts, momentum=0.75):
    """The weight curve of plot_grad_density (analyze_gradnorm.py:252-271) from its counts: 1 / the bin's population, through
    one step of the EMA from 0 when momentum > 0; 0 for an empty bin."""
    counts = np.asarray(counts, dtype=np.float64)
    acc = (1 - momentum) * counts if momentum > 0 else counts
    return np.divide(1.0, acc, out=np.zeros_like(acc), where=counts > 0)


def draw_plots(payload, plot_dir):
    """The reference's figures as step histograms: dist_<stage>.png (known / unknown / background densities),
    dist_<stage>_act.png (foreground / background) for the actionness target, grad_density.png / grad_prop_density.png
    (counts and the weight curve of plot_grad_density, momentum 0.75)."""
    import matplotlib
    matplotlib.use('Agg')
    import matplotlib.pyplot as plt
    os.makedirs(plot_dir, exist_ok=True)
    target = str(payload['target'])
    edges = payload['score_edges']
    width = np.diff(edges)

    def density(h):
        return h / max(h.sum(), 1) / width

    def steps(path, series, xlabel):
        fig = plt.figure(figsize=(5, 4))
        for h, color, name in series:
            plt.stairs(density(h.astype(np.float64)), edges, color=color, label=name, fill=True, alpha=0.4)
        plt.legend(loc='upper center')
        plt.xlabel(xlabel)
        plt.ylabel('density')
        plt.tight_layout()
        plt.savefig(path)
        plt.close(fig)

    for s, stage in enumerate(STAGES):
        known, unknown, bg = payload['hist_score'][s]
        steps(os.path.join(plot_dir, f'dist_{stage}.png'),
              [(known, 'green', 'Known'), (unknown, 'red', 'Unknown'), (bg, 'cyan', 'Background')], target)
        if target == 'actionness':
            steps(os.path.join(plot_dir, f'dist_{stage}_act.png'),
                  [(known + unknown, 'red', 'Foreground'), (bg, 'blue', 'Background')], target)
        fig, ax1 = plt.subplots(1, 1, figsize=(8, 5))
        left = payload['grad_edges'][:-1]
        ax1.step(left, payload['hist_grad'][s], 'r-', where='post', linewidth=2, label='Grad Density')
        ax1.legend(loc='upper left')
        ax2 = ax1.twinx()
        ax2.step(left, grad_weights(payload['hist_grad'][s]), 'b-', where='post', linewidth=2, label='weights')
        ax2.legend(loc='upper right')
        ax1.set_xlabel('gradient norm')
        plt.tight_layout()
        plt.savefig(os.path.join(plot_dir, 'grad_density.png' if s == 0 else 'grad_prop_density.png'))
        plt.close(fig)


def main(argv=None):
    from ..common import config as C
    from ..common.thumos_dataset import get_video_anno, get_video_info
    from .BDNet import BDNet, model_cfg_from
    own, rest = split_flags(list(sys.argv[1:] if argv is None else argv), ('--random_init', '--all_windows', '--keep_rows'),
                            {'--subset': (1, 'test'), '--target': (1, 'uncertainty'), '--output_npz': (1, None),
                             '--plots': (1, None)})
    if own['--subset'] not in ('test', 'train'):
        raise ValueError("--subset test|train")
    if own['--output_npz'] is None:
        raise ValueError("--output_npz F is required")
    config = C.set_config(C.get_config(rest))
    if 'activitynet' in str(config['dataset']['class_info_path']).lower():
        raise NotImplementedError("analyze_anchors is a THUMOS14 tool: the ActivityNet recipe matches differently and the "
                                  "reference has no such analysis for it")
    te, md, ds = config['testing'], config['model'], config['dataset']
    os_head, use_edl = md.get('os_head', False), md.get('use_edl', False)
    check_mode(own['--target'], os_head, use_edl)
    node = ds['training' if own['--subset'] == 'train' else 'testing']
    t = ds['testing']                                    # the windows run at the test stride for both subsets
    video_infos = get_video_info(node['video_info_path'])
    cls_all = os.path.join(os.path.dirname(ds['class_info_path']), 'Class_Index_All.txt')
    video_annos = get_video_anno(video_infos, node.get('video_anno_open_path', node['video_anno_path']), cls_all)
    windows = select_windows(video_infos, video_annos, t['clip_length'], t['clip_stride'], own['--all_windows'])
    rank, world, dev = device_setup()
    if world != 1:
        raise NotImplementedError("analyze_anchors runs in one process")
    net = load_net(BDNet, dev, own['--random_init'], te['checkpoint_path'], in_channels=md['in_channels'], use_edl=use_edl,
                   cfg=model_cfg_from(config))
    n_known = net.num_classes if os_head else net.num_classes - 1
    piou = config['training']['piou']
    stats = analyze(net, windows, node['video_data_path'], own['--target'], piou, n_known, t['clip_length'], t['crop_size'],
                    keep_rows=own['--keep_rows'], device=dev)
    payload = npz_payload(stats, windows, own['--target'], piou, te['split'], own['--subset'], n_known)
    os.makedirs(os.path.dirname(os.path.abspath(own['--output_npz'])), exist_ok=True)
    np.savez_compressed(own['--output_npz'], **payload)
    counts = payload['group_counts']
    print(f"{len(windows)} windows, target {own['--target']}: " + "; ".join(
        f"{stage} " + " / ".join(f"{int(counts[s, g])} {name}" for g, name in enumerate(GROUPS)) for s, stage in enumerate(STAGES))
        + f" -> {own['--output_npz']}")
    if own['--plots'] is not None:
        draw_plots(payload, own['--plots'])
    return own['--output_npz'], payload


if __name__ == '__main__':
    main()
