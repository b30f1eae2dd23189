"""Evaluation of one seeded THUMOS14-sized result set on the CPU path and on the device path.

    python tools/micro_eval.py [--videos 200] [--gts 20] [--dets 5000] [--cuda-only]

200 videos x 20 ground truths x 5 000 detections, 15 known classes (plus three unknown ones in the ground truth), tIoU
thresholds 0.3 .. 0.7, open-set protocol.  Times, with the JSON files already parsed (import is common to both paths):
  (a) ANETdetection(device='cpu'):  pre_evaluate() + evaluate('AP'), the Python loops;
  (b) ANETdetection(device='cuda'): the same two calls on a fresh evaluator -- host planners, uploads, kernel and read-back
      included -- after one tiny warm-up evaluation that loads the library and creates the device context;
and for (b) where the time goes.  Both paths must give the same lists and AP values (asserted).  (c), the kernel alone, is
what the kernel trace shows:  tools/kernel_time.sh 4 -- python tools/micro_eval.py --cuda-only
  (d) evaluate('WI') with ood_threshold 0.5 on the same set: the labelled matching on the device (upload of the labels, kernel,
      read-back; the segments are the split pass's uploads) against match_labeled_reference, the CPU rule, and the host part
      common to both (outcome flags, cumulative sums, interpolation).  Both must give the same stats and WI (asserted)."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
TIOUS = [0.3, 0.4, 0.5, 0.6, 0.7]
KNOWN = ["Known%02d" % i for i in range(15)]
UNKNOWN = ["Other%d" % i for i in range(3)]


def write_set(folder, nvideos, ngt, ndet, seed=0):
    rs = np.random.RandomState(seed)
    names = KNOWN + UNKNOWN
    database, results = {}, {}
    for v in range(nvideos):
        vid = "video_test_%07d" % v
        start = rs.uniform(0, 600, ngt)
        length = rs.uniform(2, 30, ngt)
        glabel = rs.randint(0, len(names), ngt)
        if v == 0:
            glabel[:len(names)] = np.arange(len(names))[:ngt]       # every class has ground truth
        database[vid] = {"subset": "test", "annotations": [
            {"segment": [float(start[j]), float(start[j] + length[j])], "label": names[glabel[j]]} for j in range(ngt)]}
        j = rs.randint(0, ngt, ndet)
        near = rs.rand(ndet) < 0.4
        s = np.where(near, start[j] + rs.normal(0, 0.2, ndet) * length[j], rs.uniform(0, 600, ndet))
        e = s + np.where(near, length[j] * rs.uniform(0.6, 1.5, ndet), rs.uniform(2, 30, ndet))
        label = np.where(near & (glabel[j] < len(KNOWN)) & (rs.rand(ndet) < 0.8), glabel[j], rs.randint(0, len(KNOWN), ndet))
        score, unct, act = rs.rand(ndet), rs.rand(ndet), rs.rand(ndet)
        results[vid] = [{"label": KNOWN[label[i]], "score": float(score[i]), "segment": [float(s[i]), float(e[i])],
                         "uncertainty": float(unct[i]), "actionness": float(act[i])} for i in range(ndet)]
    os.makedirs(folder, exist_ok=True)
    with open(os.path.join(folder, "classes.txt"), "w") as f:
        f.write("".join("%d %s\n" % (i + 1, n) for i, n in enumerate(KNOWN)))
    json.dump({"database": database}, open(os.path.join(folder, "gt.json"), "w"))
    json.dump({"version": "synthetic", "results": results, "external_data": {}}, open(os.path.join(folder, "pred.json"), "w"))
    open(os.path.join(folder, "done"), "w").close()


def evaluator(folder, device):
    from opental_amd.evaluation.eval_detection import ANETdetection
    return ANETdetection(ground_truth_filename=os.path.join(folder, "gt.json"), prediction_filename=os.path.join(folder, "pred.json"),
                         cls_idx_detection=os.path.join(folder, "classes.txt"), subset=["test"], openset=True,
                         ood_scoring="uncertainty", tiou_thresholds=TIOUS, device=device)


def timed(det):
    t0 = time.perf_counter()
    det.pre_evaluate()
    t1 = time.perf_counter()
    out = det.evaluate(type="AP")
    t2 = time.perf_counter()
    return t1 - t0, t2 - t1, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=200)
    ap.add_argument("--gts", type=int, default=20)
    ap.add_argument("--dets", type=int, default=5000)
    ap.add_argument("--cuda-only", action="store_true")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "micro_eval.py measures the device path: it needs a GPU"
    folder = os.path.join(tempfile.gettempdir(), "micro_eval_%d_%d_%d" % (args.videos, args.gts, args.dets))
    tiny = os.path.join(tempfile.gettempdir(), "micro_eval_2_20_50")
    for f, shape in ((folder, (args.videos, args.gts, args.dets)), (tiny, (2, 20, 50))):
        if not os.path.exists(os.path.join(f, "done")):
            write_set(f, *shape)
    timed(evaluator(tiny, "cuda"))                      # warm-up: library, device context, first launch
    evaluator(tiny, "cuda").evaluate(type="WI")         # and the labelled kernel's first launch
    t0 = time.perf_counter()
    det = evaluator(folder, "cuda")
    t_import = time.perf_counter() - t0
    n = len(det.prediction["score"])
    print("%d videos, %d ground truths, %d detections, %d tIoU thresholds; import (JSON -> columns) %.2f s"
          % (args.videos, len(det.ground_truth["label"]), n, len(TIOUS), t_import))
    split_s, ap_s, res = timed(det)
    lists = det.eval_data
    print("(b) device='cuda': pre_evaluate %.3f s + evaluate('AP') %.3f s = %.3f s   (average mAP %.6f)"
          % (split_s, ap_s, split_s + ap_s, res[1]))
    # where (b) goes: the same steps one by one on a fresh evaluator
    from opental_amd.evaluation import match
    from opental_amd.evaluation.utils_eval import interpolated_prec_rec
    fresh = evaluator(folder, "cuda")
    tick = [time.perf_counter()]
    lap = lambda: tick.append(time.perf_counter()) or tick[-1] - tick[-2]
    codes = match.video_codes(fresh.ground_truth["video-id"], fresh.prediction["video-id"]); t_codes = lap()
    sp = match.plan_split(fresh.prediction, fresh.ground_truth, codes); t_plan_s = lap()
    c_s = match.match_device(*sp.arrays(), TIOUS, plan=sp); t_dev_s = lap()
    match.split_lists(sp, c_s, fresh.prediction, fresh.ground_truth, len(TIOUS)); t_lists = lap()
    pa = match.plan_ap(fresh.prediction, fresh.ground_truth, fresh.activity_index.values(), codes); t_plan_a = lap()
    c_a = match.match_device(*pa.arrays(), TIOUS, plan=pa); t_dev_a = lap()
    match.average_precision(pa, pa.unsort(c_a), fresh.activity_index.values(), len(TIOUS), interpolated_prec_rec); t_ap = lap()
    print("    video codes %.3f s | split: planner %.3f, upload + kernel + read-back %.3f, lists %.3f | "
          "AP: planner %.3f, upload + kernel + read-back %.3f, cumsum + interpolation %.3f"
          % (t_codes, t_plan_s, t_dev_s, t_lists, t_plan_a, t_dev_a, t_ap))
    # (d) the Wilderness-Impact pass on the evaluator whose split plan is already uploaded
    det.set_ood_threshold(0.5)
    plan = det._plan("split")
    labels = (det.prediction["label"][plan.order], det.ground_truth["label"][plan.gt_order])
    pseg, pstart, gseg, gstart = plan.arrays()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    d_codes, d_top = match.match_labeled_device(pseg, labels[0], pstart, gseg, labels[1], gstart, TIOUS, plan=plan)
    t_wi_dev = time.perf_counter() - t0
    t0 = time.perf_counter()
    wi = det.evaluate(type="WI")
    t_wi_all = time.perf_counter() - t0
    print("(d) WI, device='cuda': labelled matching (labels up, kernel, read-back) %.3f s; evaluate('WI') in all %.3f s   "
          "(average WI %.6f)" % (t_wi_dev, t_wi_all, wi[1]))
    if args.cuda_only:
        return
    t0 = time.perf_counter()
    c_codes, c_top = match.match_labeled_reference(pseg, labels[0], pstart, gseg, labels[1], gstart, TIOUS)
    t_wi_cpu = time.perf_counter() - t0
    assert np.array_equal(c_codes, d_codes) and np.array_equal(c_top, d_top), "the labelled rule: device and CPU differ"
    print("(d) WI, CPU rule: match_labeled_reference %.3f s; CPU / device = %.1f" % (t_wi_cpu, t_wi_cpu / t_wi_dev))
    cpu = evaluator(folder, "cpu")
    csplit_s, cap_s, cres = timed(cpu)
    print("(a) device='cpu':  pre_evaluate %.3f s + evaluate('AP') %.3f s = %.3f s   (average mAP %.6f)"
          % (csplit_s, cap_s, csplit_s + cap_s, cres[1]))
    assert cpu.eval_data == lists, "the two paths sorted the detections differently"
    assert np.array_equal(cres[2], res[2]) and cres[1] == res[1], "the two paths give different AP"
    print("same lists, same AP; (a) / (b) = %.1f" % ((csplit_s + cap_s) / (split_s + ap_s)))


if __name__ == "__main__":
    main()
