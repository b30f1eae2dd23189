"""Evaluation driver with the reference's command line (AFSD/thumos14/eval_open.py; the closed-set branch is what
AFSD/thumos14/eval.py does for one split): per split, closed-set mAP or -- with --open_set -- AUROC / AUPR / FAR@95 /
OSDR of the result JSON written by thumos14/test.py, the per-split text files `eval.txt` / `eval_open.txt` in the
reference's format, and mean +- 1.96 sigma / sqrt(n) over the splits.

    python -m opental_amd.thumos14.eval_open output/opental/split_{id:d}/detection_results.json \\
        datasets/thumos14/annotations_open/split_{id:d}/known_gt.json --cls_idx_known .../action_known.txt \\
        --all_splits 0 1 2 --open_set --ood_scoring uncertainty_actionness [--device cuda] \\
        [--wi] [--stats_json FILE] [--ood_threshold THR]

--wi adds the Wilderness Impact (evaluate('WI'), which the reference's driver carries commented out, :77-80) to the printed
summary; --stats_json writes the open-set error breakdown of every split: per tIoU threshold the number of detections in each
of the seven outcomes (and in none) and the mean and 1.96 sigma / sqrt(n) of their out-of-distribution scores -- the numbers
behind the reference's experiments/analyze_stats.py:37-80, as that script counts them: `fp_k2u` / `fp_k2k` include the
background detections `fp_bg2u` / `fp_bg2k`.  --ood_threshold relabels detections whose score is below it as '__unknown__'
(ANETdetection's ood_threshold) for result files that do not carry the label themselves.
"""
import argparse
import json
import os

import numpy as np

from ..evaluation.eval_detection import ANETdetection


def write_eval_open(eval_file, tious, far_95, auc_ROC, auc_PR, OSDR):
    with open(eval_file, 'w') as f:
        for (tiou, far, auc_roc, auc_pr, osdr) in zip(tious, far_95, auc_ROC, auc_PR, OSDR):
            f.writelines(f"tIoU={tiou}: far@95={far:.5f}, auc_roc={auc_roc:.5f}, auc_pr={auc_pr:.5f}, osdr={osdr:.5f}\n")
        f.writelines(f"Average FAR@95: {far_95.mean():.5f}, Average AUC_ROC: {auc_ROC.mean():.5f}, "
                     f"Average AUC_PR: {auc_PR.mean():.5f}, Average OSDR: {OSDR.mean():.5f}\n")


def write_eval_closed(eval_file, tious, mAPs, average_mAP):
    with open(eval_file, 'w') as f:
        for (tiou, mAP) in zip(tious, mAPs):
            f.writelines(f"tIoU={tiou}: mAP={mAP:.5f}\n")
        f.writelines(f"Average mAP: {average_mAP:.5f}\n")


def get_mean_std(data, axis=0):
    """Mean and 95 % confidence half-width over splits (eval_open.py:104-108)."""
    mean = np.array(data).mean(axis=axis)
    std = np.array(data).std(axis=axis) / np.sqrt(len(data)) * 1.96
    return mean, std


STATS_OUTCOMES = ('tp_u2u', 'tp_k2k', 'fp_u2k', 'fp_k2k', 'fp_k2u', 'fp_bg2u', 'fp_bg2k')


def error_breakdown(stats, tious):
    """ANETdetection.stats -> per tIoU threshold the detections per outcome ('none': flagged in no array) and the mean and
    95 % half-width of their out-of-distribution scores (analyze_stats.py:37-80; null for an outcome without detections)."""
    ood = np.asarray(stats['ood_scores'], dtype=np.float64)
    rows = []
    for tidx, tiou in enumerate(tious):
        masks = {k: (stats[k][tidx].sum(axis=0) if stats[k][tidx].ndim == 2 else stats[k][tidx]) > 0 for k in STATS_OUTCOMES}
        flagged = np.zeros(len(ood), dtype=bool)
        for m in masks.values():
            flagged |= m
        masks['none'] = ~flagged
        row = {'tiou': float(tiou), 'counts': {k: int(m.sum()) for k, m in masks.items()}, 'ood_mean': {}, 'ood_ci': {}}
        for k, m in masks.items():
            n = int(m.sum())
            row['ood_mean'][k] = float(np.mean(ood[m])) if n else None
            row['ood_ci'][k] = float(np.std(ood[m]) / np.sqrt(n) * 1.96) if n else None
        rows.append(row)
    return {'detections': int(len(ood)), 'num_gt': [int(x) for x in stats['num_gt']], 'thresholds': rows}


def evaluate_split(pred_file, gt_file, cls_idx_known, tious, subset, open_set, ood_scoring='confidence', dataset='thumos14',
                   write=True, device='cpu', wi=False, ood_threshold=None):
    """-> the split's metrics; with `wi` (open set only) also 'wi' = mean WI per tIoU and 'stats' = error_breakdown."""
    det = ANETdetection(ground_truth_filename=gt_file, prediction_filename=pred_file, cls_idx_detection=cls_idx_known,
                        subset=subset, openset=open_set, ood_scoring=ood_scoring, tiou_thresholds=tious, dataset=dataset,
                        device=device, ood_threshold=ood_threshold)
    if open_set:
        det.pre_evaluate()
        auc_ROC, auc_PR, far_95 = det.evaluate(type='AUC')
        OSDR = det.evaluate(type='OSDR')
        if write:
            write_eval_open(os.path.join(os.path.dirname(pred_file), 'eval_open.txt'), tious, far_95, auc_ROC, auc_PR, OSDR)
        out = {'far_95': far_95, 'auc_roc': auc_ROC, 'auc_pr': auc_PR, 'osdr': OSDR}
        if wi:
            out['wi'] = det.evaluate(type='WI')[0]
            out['stats'] = error_breakdown(det.stats, tious)
        return out
    mAPs, average_mAP, _ = det.evaluate(type='AP')
    if write:
        write_eval_closed(os.path.join(os.path.dirname(pred_file), 'eval.txt'), tious, mAPs, average_mAP)
    return {'mAP': mAPs, 'average_mAP': average_mAP}


def print_summary(per_split, tious, open_set):
    """Mean and confidence half-width over the splits, per tIoU and of the per-split averages; shared with
    opental_amd.anet.eval_open."""
    names = (('far_95', 'FAR@95'), ('auc_roc', 'AUC_ROC'), ('auc_pr', 'AUC_PR'), ('osdr', 'OSDR')) if open_set else (('mAP', 'mAP'),)
    if open_set and all('wi' in r for r in per_split):
        names += (('wi', 'WI'),)
    for key, title in names:
        mean, std = get_mean_std([r[key] for r in per_split])
        avg_mean, avg_std = get_mean_std([np.mean(r[key]) for r in per_split])
        for tiou, m, s in zip(tious, mean, std):
            print(f"{title}(tIoU={tiou}): mean={m:.5f}, std={s:.5f}")
        print(f"Average {title} = {avg_mean:.5f} ({avg_std:.5f})\n")


def add_wi_arguments(parser):
    """--wi / --stats_json / --ood_threshold; shared with opental_amd.anet.eval_open."""
    parser.add_argument('--wi', action='store_true', help='open set: also the Wilderness Impact per tIoU and its average')
    parser.add_argument('--stats_json', type=str, default=None,
                        help='open set: write the error breakdown (detections and mean OOD score per outcome) of every split')
    parser.add_argument('--ood_threshold', type=float, default=None,
                        help="open set: detections with an OOD score below it are relabelled '__unknown__'")


def check_wi_arguments(parser, args):
    if (args.wi or args.stats_json or args.ood_threshold is not None) and not args.open_set:
        parser.error('--wi, --stats_json and --ood_threshold belong to the open-set protocol: add --open_set')


def finish_wi(per_split, args):
    """Write --stats_json and keep 'wi' in the summary only where --wi asked for it."""
    if args.stats_json:
        with open(args.stats_json, 'w') as f:
            json.dump({'ood_scoring': args.ood_scoring, 'ood_threshold': args.ood_threshold,
                       'splits': {str(split): r['stats'] for split, r in zip(args.all_splits, per_split)}}, f, indent=1)
    if not args.wi:
        for r in per_split:
            r.pop('wi', None)


def main(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument('output_json', type=str)
    parser.add_argument('gt_json', type=str, default='datasets/thumos14/annotations/thumos_gt.json', nargs='?')
    parser.add_argument('--cls_idx_known', type=str)
    parser.add_argument('--all_splits', nargs='+', type=int)
    parser.add_argument('--open_set', action='store_true')
    parser.add_argument('--dataset', type=str, default='thumos14', choices=['thumos14', 'thumos_anet'])
    parser.add_argument('--ood_scoring', type=str, default='confidence',
                        choices=['uncertainty', 'confidence', 'uncertainty_actionness', 'a_by_inv_u', 'u_by_inv_a', 'half_au'])
    parser.add_argument('--device', type=str, default='cpu', choices=['cpu', 'cuda'],
                        help='cuda: the matching passes run through the device kernel (evaluation/match.py)')
    add_wi_arguments(parser)
    args = parser.parse_args(argv)
    check_wi_arguments(parser, args)
    tious = np.linspace(0.5, 0.95, 10) if args.dataset == 'thumos_anet' else [0.3, 0.4, 0.5, 0.6, 0.7]
    subset = ['test', 'validation'] if args.dataset == 'thumos_anet' else ['test']
    per_split = []
    for split in args.all_splits:
        gt_file = args.gt_json if args.open_set else args.gt_json.format(id=split)
        per_split.append(evaluate_split(args.output_json.format(id=split), gt_file, args.cls_idx_known.format(id=split),
                                        tious, subset, args.open_set, args.ood_scoring, args.dataset, device=args.device,
                                        wi=args.wi or bool(args.stats_json), ood_threshold=args.ood_threshold))
    finish_wi(per_split, args)
    print_summary(per_split, tious, args.open_set)
    return per_split


if __name__ == '__main__':
    main()
