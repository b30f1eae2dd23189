"""Detection tables -> AP on the device against the result-JSON route, on one seeded THUMOS14-sized result set.

    python tools/micro_table_ap.py [--videos 200] [--gts 20] [--dets 5000] [--batch 8]

200 videos x 20 ground truths x 5 000 detections, 15 classes, tIoU thresholds 0.3 .. 0.7, closed-set protocol; scores are
distinct inside every class (the condition under which the host's argsort()[::-1] is determined).  The detections sit on the
device as the tables of ops.detection_table's layout, one per batch of videos, which is where
opental_amd.common.score_checkpoints has them.  Times, after one tiny warm-up of each route:
  (a) table_ap(tables, ground truth, thresholds): the torch sorts and offsets, otal_eval_match, otal_average_precision, the
      read-back of the AP array -- what one checkpoint costs after its forward passes; the median of five calls after one
      untimed call of the same shape;
  (b) the route of the parent tree from the same detections: proposal dicts from the tables (proposals_from_table), the result
      JSON written, ANETdetection(device='cuda') reading it, evaluate('AP') (host planner, matching kernel, AP arithmetic on the
      host), each step on its own, once (ten seconds of host work).
There is no gate on the ratio.  The two AP arrays must agree within table_ap.tolerance(npos), 4 npos 2^-53; otherwise nothing
is reported and the exit status is 1."""
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
TIOUS = [0.3, 0.4, 0.5, 0.6, 0.7]
CLASSES = ["Known%02d" % i for i in range(15)]
REPEATS = 5


def make_set(nvideos, ngt, ndet, seed=0):
    """-> (det columns in (video, class) order, gt columns): about 40 % of the detections are jittered copies of a ground truth
    of their video, most of those with its class."""
    rs = np.random.RandomState(seed)
    K = len(CLASSES)
    gv, gc, gs, dv, dc, ds = [], [], [], [], [], []
    for v in range(nvideos):
        start, length = rs.uniform(0, 600, ngt), rs.uniform(2, 30, ngt)
        glabel = rs.randint(0, K, ngt)
        if v == 0:
            glabel[:K] = np.arange(K)[:ngt]                 # every class has ground truth
        j = rs.randint(0, ngt, ndet)
        near = rs.rand(ndet) < 0.4
        s = np.where(near, start[j] + rs.normal(0, 0.2, ndet) * length[j], rs.uniform(0, 600, ndet))
        e = s + np.where(near, length[j] * rs.uniform(0.6, 1.5, ndet), rs.uniform(2, 30, ndet))
        label = np.where(near & (rs.rand(ndet) < 0.8), glabel[j], rs.randint(0, K, ndet))
        order = np.argsort(label, kind='stable')
        gv.append(np.full(ngt, v)); gc.append(glabel); gs.append(np.stack([start, start + length], 1))
        dv.append(np.full(ndet, v)); dc.append(label[order]); ds.append(np.stack([s, e], 1)[order])
    n = nvideos * ndet
    score = ((rs.permutation(n) + 1.0) / (n + 1.0)).astype(np.float32)
    assert n < 2 ** 23 and len(np.unique(score)) == n
    det = dict(video=np.concatenate(dv).astype(np.int32), cls=np.concatenate(dc).astype(np.int32), seg=np.concatenate(ds),
               score=score)
    gt = dict(video=np.concatenate(gv).astype(np.int32), cls=np.concatenate(gc).astype(np.int32), seg=np.concatenate(gs))
    return det, gt


def device_tables(det, nvideos, batch, device):
    """One table per `batch` videos, in ops.detection_table's layout with list_start, `video` local to the batch."""
    import torch
    K = len(CLASSES)
    tables, firsts = [], []
    for v0 in range(0, nvideos, batch):
        rows = np.flatnonzero((det['video'] >= v0) & (det['video'] < v0 + batch))
        V = min(batch, nvideos - v0)
        key = (det['video'][rows] - v0) * K + det['cls'][rows]
        sup = np.zeros((len(rows), 3), dtype=np.float32)
        sup[:, 0] = det['score'][rows]
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
        tables.append(dict(video=up(det['video'][rows] - v0), cls=up(det['cls'][rows]), seg=up(det['seg'][rows]), sup=up(sup),
                           list_start=up(np.searchsorted(key, np.arange(V * K + 1)).astype(np.int32)),
                           n=torch.tensor(len(rows), dtype=torch.int32, device=device)))
        firsts.append(v0)
    return tables, firsts


def ground_truth(gt, nvideos):
    from opental_amd.evaluation.table_ap import GroundTruth
    return GroundTruth(gt['video'], gt['cls'], gt['seg'], len(CLASSES), {"video_test_%07d" % v: v for v in range(nvideos)})


def device_route(det, gt, nvideos, batch, device):
    """-> (seconds of each of `REPEATS` calls after one untimed call of the same shape, ap): table_ap on tables that are
    already on the device and numbered.  The call ends in the read-back of the AP array, which waits for the device."""
    import torch
    from opental_amd.evaluation.table_ap import table_ap
    tables, firsts = device_tables(det, nvideos, batch, device)
    for t, v0 in zip(tables, firsts):
        t['video'] += v0
    truth = ground_truth(gt, nvideos)
    truth.device_arrays(device)                     # uploaded once per run of the driver, not per checkpoint
    ap = table_ap(tables, truth, TIOUS)
    times = []
    for _ in range(REPEATS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        again = table_ap(tables, truth, TIOUS)
        times.append(time.perf_counter() - t0)
        assert again.tobytes() == ap.tobytes(), "table_ap is not repeatable"
    return times, ap


def json_route(det, gt, nvideos, batch, device, folder):
    """-> (dict of seconds per step, ap): the parent tree's route from the same tables."""
    import torch
    from opental_amd.common.det_table import proposals_from_table
    from opental_amd.common.detect import results_json
    from opental_amd.evaluation.eval_detection import ANETdetection
    os.makedirs(folder, exist_ok=True)
    database = {}
    for v, c, seg in zip(gt['video'].tolist(), gt['cls'].tolist(), gt['seg'].tolist()):
        database.setdefault("video_test_%07d" % v, dict(subset="test", annotations=[]))['annotations'].append(
            dict(label=CLASSES[c], segment=seg))
    paths = [os.path.join(folder, n) for n in ("gt.json", "pred.json", "classes.txt")]
    json.dump(dict(database=database), open(paths[0], "w"))
    with open(paths[2], "w") as f:
        f.write("".join("%d %s\n" % (i + 1, n) for i, n in enumerate(CLASSES)))
    tables, firsts = device_tables(det, nvideos, batch, device)
    idx_to_class = {i + 1: n for i, n in enumerate(CLASSES)}
    torch.cuda.synchronize()
    tick = [time.perf_counter()]
    lap = lambda: tick.append(time.perf_counter()) or tick[-1] - tick[-2]
    results = {}
    for t, v0 in zip(tables, firsts):
        V = (t['list_start'].numel() - 1) // len(CLASSES)
        results.update(proposals_from_table(t, ["video_test_%07d" % (v0 + v) for v in range(V)], idx_to_class))
    steps = dict(dicts=lap())
    json.dump(results_json(results), open(paths[1], "w"))
    steps['write'] = lap()
    evaluator = ANETdetection(ground_truth_filename=paths[0], prediction_filename=paths[1], cls_idx_detection=paths[2],
                              subset=["test"], tiou_thresholds=TIOUS, device='cuda')
    steps['read'] = lap()
    ap = evaluator.evaluate('AP')[2]
    steps['evaluate'] = lap()
    return steps, ap


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--videos", type=int, default=200)
    p.add_argument("--gts", type=int, default=20)
    p.add_argument("--dets", type=int, default=5000)
    p.add_argument("--batch", type=int, default=8)
    args = p.parse_args()
    import torch
    from opental_amd.evaluation.table_ap import tolerance
    assert torch.cuda.is_available(), "micro_table_ap.py measures the device path: it needs a GPU"
    device = torch.device("cuda", 0)
    folder = tempfile.mkdtemp(prefix="micro_table_ap_")
    tiny = make_set(2, 20, 50, seed=1)
    device_route(*tiny, 2, args.batch, device)              # warm-up: library, device context, first launches
    json_route(*tiny, 2, args.batch, device, os.path.join(folder, "tiny"))
    det, gt = make_set(args.videos, args.gts, args.dets)
    times, ap_dev = device_route(det, gt, args.videos, args.batch, device)
    t_dev = float(np.median(times))
    steps, ap_json = json_route(det, gt, args.videos, args.batch, device, os.path.join(folder, "set"))
    shutil.rmtree(folder, ignore_errors=True)
    npos = int(np.bincount(gt['cls']).max())
    err = float(np.abs(ap_dev - ap_json).max())
    if not err <= tolerance(npos):
        print("the two routes give different AP: max |dAP| %.3e > %.3e (npos %d); no times reported" % (err, tolerance(npos), npos))
        return 1
    t_json = sum(steps.values())
    print("%d videos, %d ground truths, %d detections in %d tables, %d tIoU thresholds; average mAP %.6f, max |dAP| %.1e"
          % (args.videos, len(gt['cls']), len(det['cls']), -(-args.videos // args.batch), len(TIOUS), ap_dev.mean(), err))
    print("(a) tables -> AP on the device (table_ap): median %.4f s of %d calls (%.4f .. %.4f)"
          % (t_dev, len(times), min(times), max(times)))
    print("(b) tables -> dicts %.3f s, result JSON written %.3f s, read by ANETdetection %.3f s, evaluate('AP') with "
          "device='cuda' %.3f s: %.3f s" % (steps['dicts'], steps['write'], steps['read'], steps['evaluate'], t_json))
    print("(b) / (a) = %.0f" % (t_json / t_dev))
    return 0


if __name__ == "__main__":
    sys.exit(main())
