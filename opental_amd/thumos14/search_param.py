"""Search of the open-set threshold that maximises the average mAP (AFSD/thumos14/search_param.py:210-275).

    python -m opental_amd.thumos14.search_param <yaml> --open_set --split N [--device cuda]

Ten candidates np.arange(0.8, 1.0, 0.02); each is used directly as the open-set threshold (`ood_thresh = param`, :213) of an
evaluation at the tIoU thresholds 0.3 .. 0.7, printed as the reference prints it, then the best one.  The detections are the
result file <output_path>/<output_json> where it exists, otherwise one thumos14.test run writes it.  The reference caches raw
network outputs in raw_outputs.npz and writes one result JSON per candidate, although its post_process ignores `param`
apart from the file name: every candidate sees the same detections, so the search here is ONE evaluator and
ANETdetection.set_ood_threshold per candidate -- neither the cache nor the JSON round trip is restated.  With
`--device cuda` the ten AP passes run through the device matching kernel (evaluation/match.py)."""
import os
import sys

import numpy as np

from ..evaluation.eval_detection import ANETdetection

TIOUS = [0.3, 0.4, 0.5, 0.6, 0.7]
GT_KNOWN_JSON = 'datasets/thumos14/annotations_open/split_{id:d}/known_gt.json'     # search_param.py:53
GT_ALL_JSON = 'datasets/thumos14/annotations/thumos_gt.json'                        # search_param.py:54


def candidates():
    return np.arange(0.8, 1.0, step=0.02)


def search(det, candidates, verbose=False):
    """The loop of search_param.py:266-274 on one evaluator -> (best_param, best_mAP, all_mAPs)."""
    all_mAPs = []
    for param in candidates:
        det.set_ood_threshold(param)
        _, average_mAP, _ = det.evaluate(type='AP')
        if verbose:
            print(f'Param: {param:.3f}, OOD threshold: {param:.6f}, Average mAP: {average_mAP*100:.3f}%')
        all_mAPs.append(average_mAP)
    idx = int(np.array(all_mAPs).argmax())
    return candidates[idx], all_mAPs[idx], all_mAPs


def main(argv=None):
    from ..common import config as C
    argv = list(sys.argv[1:] if argv is None else argv)
    device = 'cpu'
    if '--device' in argv:
        i = argv.index('--device')
        device = argv[i + 1]
        del argv[i:i + 2]
    if device not in ('cpu', 'cuda'):
        raise SystemExit("--device is cpu or cuda")
    config = C.get_config(argv)
    te = config['testing']
    pred_file = os.path.join(te['output_path'], te['output_json'])
    if not os.path.exists(pred_file):
        from . import test
        test.main(argv)
    gt_file = GT_ALL_JSON if config['open_set'] else GT_KNOWN_JSON.format(id=te['split'])     # search_param.py:254
    det = ANETdetection(ground_truth_filename=gt_file, prediction_filename=pred_file,
                        cls_idx_detection=config['dataset']['class_info_path'], subset=['test'], openset=config['open_set'],
                        ood_scoring=te['ood_scoring'], tiou_thresholds=TIOUS, verbose=False, device=device)
    cand = candidates()
    best_param, best_mAP, all_mAPs = search(det, cand, verbose=True)
    print(f'\nBest Param: {best_param:.3f}, Current OOD threshold: {best_param:.6f}, Best Average mAP: {best_mAP*100:.3f}%')
    return best_param, best_mAP, all_mAPs


if __name__ == '__main__':
    main()
