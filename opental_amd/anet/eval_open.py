"""Evaluation driver of the ActivityNet1.3 recipe, with the command line of opental_amd.thumos14.eval_open
(AFSD/anet/eval_open.py; without --open_set it is what AFSD/anet/eval.py does, per split): closed-set mAP or -- with
--open_set -- FAR@95 / AUROC / AUPR / OSDR of the result JSON written by anet/test.py, the per-split text files `eval.txt` /
`eval_open.txt`, and mean +- 1.96 sigma / sqrt(n) over the splits.

    python -m opental_amd.anet.eval_open output/anet/opental/split_{id:d}/detection_results.json \\
        datasets/activitynet/annotations_open/split_{id:d}/known_gt.json \\
        --cls_idx_known datasets/activitynet/annotations_open/split_{id:d}/action_known.txt \\
        --all_splits 0 1 2 --open_set --ood_scoring uncertainty_actionness [--device cuda] [--tious 0.1 0.2 0.3 0.4 0.5] \\
        [--wi] [--stats_json FILE] [--ood_threshold THR]

Differences from the THUMOS14 driver: dataset 'anet' (one class name per line), the `validation` subset, a ground-truth path
formatted with the split id in both protocols (:39), and --tious (--wi, --stats_json and --ood_threshold are the THUMOS14
driver's).  The default list is ActivityNet's
np.linspace(0.5, 0.95, 10) (anet/eval.py:11); the reference's open-set script carries 0.1 .. 0.5 (:16), a leftover of the
THUMOS14 file it was copied from, which --tious selects.  That script also unpacks two values from evaluate('AUC'), which
returns three (:64), so it does not run as shipped; the text files therefore have the line format of the THUMOS14 driver, the
one place where the reference writes FAR@95."""
import argparse

import numpy as np

from ..thumos14.eval_open import add_wi_arguments, check_wi_arguments, evaluate_split, finish_wi, print_summary

SUBSET = ['validation']


def default_tious():
    return np.linspace(0.5, 0.95, 10)


def main(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument('output_json', type=str)
    parser.add_argument('gt_json', type=str, default='datasets/activitynet/annotations/activity_net_1_3_new.json', nargs='?')
    parser.add_argument('--cls_idx_known', type=str)
    parser.add_argument('--all_splits', nargs='+', type=int)
    parser.add_argument('--open_set', action='store_true')
    parser.add_argument('--ood_scoring', type=str, default='confidence',
                        choices=['uncertainty', 'confidence', 'uncertainty_actionness', 'a_by_inv_u', 'u_by_inv_a', 'half_au'])
    parser.add_argument('--device', type=str, default='cpu', choices=['cpu', 'cuda'],
                        help='cuda: the matching passes run through the device kernel (evaluation/match.py)')
    parser.add_argument('--tious', nargs='+', type=float, default=None,
                        help='tIoU thresholds; default: 0.5 .. 0.95 in ten steps')
    add_wi_arguments(parser)
    args = parser.parse_args(argv)
    check_wi_arguments(parser, args)
    tious = default_tious() if args.tious is None else np.array(args.tious, dtype=np.float64)
    per_split = []
    for split in args.all_splits:
        per_split.append(evaluate_split(args.output_json.format(id=split), args.gt_json.format(id=split),
                                        args.cls_idx_known.format(id=split), tious, SUBSET, args.open_set, args.ood_scoring,
                                        'anet', device=args.device, wi=args.wi or bool(args.stats_json),
                                        ood_threshold=args.ood_threshold))
    finish_wi(per_split, args)
    print_summary(per_split, tious, args.open_set)
    return per_split


if __name__ == '__main__':
    main()
