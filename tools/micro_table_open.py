"""Detection tables -> AUROC / AUPR / FAR@95 / OSDR on the device against the result-JSON route, on one seeded THUMOS14-sized
result set.

    python tools/micro_table_open.py [--videos 200] [--gts 20] [--dets 5000] [--batch 8]

The set of tools/micro_table_ap.py -- 200 videos x 20 ground truths x 5 000 detections, 15 classes, tIoU 0.3 .. 0.7 -- in the
open-set protocol: about 40 % of the ground truths carry a label outside the class list, and every detection has an
uncertainty that is a distinct multiple of 2^-20 (so `1 - x` is exact and the host's unstable argsort has no ties to decide).
The detections sit on the device as the tables of ops.detection_table's layout, one per batch of videos.  Times, after one tiny
warm-up of each route:
  (a) table_open(tables, ground truth, thresholds): the torch sorts and offsets, otal_eval_match with group = video, the scatter,
      otal_open_set_curves, the read-back -- what the four numbers cost per checkpoint after its forward passes; the median of
      five calls after one untimed call of the same shape;
  (b) the route through the files from the same detections: proposal dicts from the tables (proposals_from_table), the result
      JSON written, ANETdetection(openset=True, device='cuda') reading it, pre_evaluate, evaluate('AUC') and evaluate('OSDR'),
      each step on its own, once.
There is no gate on the ratio.  The host stores float32: the device's numbers cast to float32 must be within one float32 ulp of
the host's and FAR@95 equal; otherwise nothing is reported and the exit status is 1."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import micro_table_ap as A     # noqa: E402  (the set, its class list and its thresholds)

REPEATS = 5
SCORING = 'uncertainty'


def make_set(nvideos, ngt, ndet, seed=0):
    """micro_table_ap's set with unknown ground truths (cls = -1, about 40 %) and an `uncertainty` column: distinct multiples
    of 2^-20 below 1."""
    det, gt = A.make_set(nvideos, ngt, ndet, seed)
    rs = np.random.RandomState(seed + 1000)
    n = len(det['cls'])
    assert n < 2 ** 20
    det['uncertainty'] = ((rs.permutation(2 ** 20 - 1)[:n] + 1.0) / 2.0 ** 20).astype(np.float32)
    gt['cls'] = np.where(rs.rand(len(gt['cls'])) < 0.4, -1, gt['cls']).astype(np.int32)
    return det, gt


def device_tables(det, nvideos, batch, device):
    """micro_table_ap's tables with the uncertainty in sup[:, 1] and the `known` column, 1 - uncertainty in fp64."""
    import torch
    tables, firsts = A.device_tables(det, nvideos, batch, device)
    for t, v0 in zip(tables, firsts):
        rows = np.flatnonzero((det['video'] >= v0) & (det['video'] < v0 + batch))
        u = torch.from_numpy(det['uncertainty'][rows]).to(device)
        t['sup'][:, 1] = u
        t['known'] = 1.0 - u.double()
    return tables, firsts


def device_route(det, gt, nvideos, batch, device):
    """-> (seconds of each of `REPEATS` calls after one untimed call of the same shape, the four arrays): table_open on tables
    that are already on the device and numbered.  The call ends in the read-back of the result, which waits for the device."""
    import torch
    from opental_amd.evaluation.table_open import KEYS, table_open
    tables, firsts = device_tables(det, nvideos, batch, device)
    for t, v0 in zip(tables, firsts):
        t['video'] += v0
    truth = A.ground_truth(gt, nvideos)
    truth.split_arrays(device)                      # uploaded once per run of the driver, not per checkpoint
    first = table_open(tables, truth, A.TIOUS)
    times = []
    for _ in range(REPEATS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        again = table_open(tables, truth, A.TIOUS)
        times.append(time.perf_counter() - t0)
        assert all(again[k].tobytes() == first[k].tobytes() for k in KEYS), "table_open is not repeatable"
    return times, first


def json_route(det, gt, nvideos, batch, device, folder):
    """-> (dict of seconds per step, the host's four float32 arrays): the route through the files from the same tables."""
    import torch
    from opental_amd.common.det_table import proposals_from_table
    from opental_amd.common.detect import results_json
    from opental_amd.evaluation.eval_detection import ANETdetection
    os.makedirs(folder, exist_ok=True)
    database = {}
    for v, c, seg in zip(gt['video'].tolist(), gt['cls'].tolist(), gt['seg'].tolist()):
        database.setdefault("video_test_%07d" % v, dict(subset="test", annotations=[]))['annotations'].append(
            dict(label=A.CLASSES[c] if c >= 0 else "NotInTheList", segment=seg))
    paths = [os.path.join(folder, n) for n in ("gt.json", "pred.json", "classes.txt")]
    json.dump(dict(database=database), open(paths[0], "w"))
    with open(paths[2], "w") as f:
        f.write("".join("%d %s\n" % (i + 1, n) for i, n in enumerate(A.CLASSES)))
    tables, firsts = device_tables(det, nvideos, batch, device)
    idx_to_class = {i + 1: n for i, n in enumerate(A.CLASSES)}
    torch.cuda.synchronize()
    tick = [time.perf_counter()]
    lap = lambda: tick.append(time.perf_counter()) or tick[-1] - tick[-2]
    results = {}
    for t, v0 in zip(tables, firsts):
        V = (t['list_start'].numel() - 1) // len(A.CLASSES)
        results.update(proposals_from_table(t, ["video_test_%07d" % (v0 + v) for v in range(V)], idx_to_class))
    steps = dict(dicts=lap())
    json.dump(results_json(results), open(paths[1], "w"))
    steps['write'] = lap()
    evaluator = ANETdetection(ground_truth_filename=paths[0], prediction_filename=paths[1], cls_idx_detection=paths[2],
                              subset=["test"], tiou_thresholds=A.TIOUS, openset=True, ood_scoring=SCORING, device='cuda')
    steps['read'] = lap()
    evaluator.pre_evaluate()
    steps['split'] = lap()
    auroc, aupr, far = evaluator.evaluate('AUC')
    steps['auc'] = lap()
    osdr = evaluator.evaluate('OSDR')
    steps['osdr'] = lap()
    return steps, dict(auroc=auroc, aupr=aupr, far95=far, osdr=osdr)


def agree(dev, host):
    """The device's fp64 numbers against the host's float32 ones: (within one float32 ulp and FAR@95 equal, the largest
    difference in ulps)."""
    worst, ok = 0.0, True
    for k in ('auroc', 'aupr', 'osdr'):
        ulps = np.abs(dev[k].astype(np.float32) - host[k]) / np.spacing(np.abs(host[k]))
        worst = max(worst, float(ulps.max()))
        ok = ok and bool((ulps <= 1).all())
    return ok and np.array_equal(dev['far95'].astype(np.float32), host['far95'], equal_nan=True), worst


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--videos", type=int, default=200)
    p.add_argument("--gts", type=int, default=20)
    p.add_argument("--dets", type=int, default=5000)
    p.add_argument("--batch", type=int, default=8)
    args = p.parse_args()
    import torch
    assert torch.cuda.is_available(), "micro_table_open.py measures the device path: it needs a GPU"
    device = torch.device("cuda", 0)
    folder = tempfile.mkdtemp(prefix="micro_table_open_")
    tiny = make_set(2, 20, 50, seed=1)
    device_route(*tiny, 2, args.batch, device)              # warm-up: library, device context, first launches
    json_route(*tiny, 2, args.batch, device, os.path.join(folder, "tiny"))
    det, gt = make_set(args.videos, args.gts, args.dets)
    times, dev = device_route(det, gt, args.videos, args.batch, device)
    t_dev = float(np.median(times))
    steps, host = json_route(det, gt, args.videos, args.batch, device, os.path.join(folder, "set"))
    shutil.rmtree(folder, ignore_errors=True)
    ok, worst = agree(dev, host)
    if not ok:
        print("the two routes give different numbers (largest difference %.2f float32 ulps, FAR@95 %s vs %s); no times reported"
              % (worst, dev['far95'].tolist(), host['far95'].tolist()))
        return 1
    t_json = sum(steps.values())
    print("%d videos, %d ground truths (%d unknown), %d detections in %d tables, %d tIoU thresholds"
          % (args.videos, len(gt['cls']), int((gt['cls'] < 0).sum()), len(det['cls']), -(-args.videos // args.batch), len(A.TIOUS)))
    print("mean AUROC %.6f AUPR %.6f FAR@95 %.6f OSDR %.6f; largest difference from the host's float32: %.2f ulps"
          % (dev['auroc'].mean(), dev['aupr'].mean(), dev['far95'].mean(), dev['osdr'].mean(), worst))
    print("(a) tables -> the four numbers on the device (table_open): median %.4f s of %d calls (%.4f .. %.4f)"
          % (t_dev, len(times), min(times), max(times)))
    print("(b) tables -> dicts %.3f s, result JSON written %.3f s, read by ANETdetection %.3f s, pre_evaluate with device='cuda' "
          "%.3f s, evaluate('AUC') %.3f s, evaluate('OSDR') %.3f s: %.3f s"
          % (steps['dicts'], steps['write'], steps['read'], steps['split'], steps['auc'], steps['osdr'], t_json))
    print("(b) / (a) = %.0f" % (t_json / t_dev))
    return 0


if __name__ == "__main__":
    sys.exit(main())
