"""Shared inputs of test_table_ap_cpu.py / test_table_ap_gpu.py: seeded (det, gt) column sets in the layout of
opental_amd/evaluation/table_ap.py, the same sets written through the evaluator's JSON layout, and device tables cut from
them.  TILE is the AP kernel's workgroup tile, from the one constant the wrapper exports."""
import json
import os

import numpy as np

from opental_amd.common.ops import AP_TILE as TILE

TIOUS = [0.3, 0.4, 0.5, 0.6, 0.7]
THRESHOLD_SETS = {1: [0.5], 10: np.linspace(0.5, 0.95, 10).tolist(), 32: np.linspace(0.05, 0.98, 32).tolist()}
CLASS_SIZES = (1, TILE - 1, TILE, TILE + 1, 2 * TILE + 3)


def _pack(name, n_classes, det_rows, gt_rows, thresholds=TIOUS, host=True):
    """det_rows of (video, cls, start, end, score), gt_rows of (video, cls, start, end) -> a case.  Detections are put in the
    table's (video, class) order, rows of one list in the order given.  host: the host evaluator's result is determined
    (distinct scores inside every class, no two ground truths whose equal tIoU decides a later match)."""
    det_rows = sorted(det_rows, key=lambda r: (r[0], r[1]))         # stable
    det = dict(video=np.array([r[0] for r in det_rows], dtype=np.int32), cls=np.array([r[1] for r in det_rows], dtype=np.int32),
               seg=np.array([r[2:4] for r in det_rows], dtype=np.float64).reshape(-1, 2),
               score=np.array([r[4] for r in det_rows], dtype=np.float32))
    gt = dict(video=np.array([r[0] for r in gt_rows], dtype=np.int32), cls=np.array([r[1] for r in gt_rows], dtype=np.int32),
              seg=np.array([r[2:4] for r in gt_rows], dtype=np.float64).reshape(-1, 2))
    return dict(name=name, n_classes=n_classes, det=det, gt=gt, thresholds=list(thresholds), host=host)


def _distinct_scores(rs, det_rows):
    """Scores (k + 1) / (n + 1), a random permutation over ALL rows: distinct as fp32 inside every class."""
    n = len(det_rows)
    perm = rs.permutation(n)
    return [r[:4] + (float(np.float32((perm[i] + 1.0) / (n + 1.0))),) for i, r in enumerate(det_rows)]


def random_case(name, seed, n_classes, n_videos, det_counts, gt_per_group=(0, 3), thresholds=TIOUS, orphan_video=True,
                all_fp=(), all_tp=()):
    """Random segments: every (class, video) group gets gt_per_group[0] .. [1] ground truths (the class's first video at least
    one), class c gets det_counts[c] detections over random videos, about half of them jittered copies of a ground truth of
    their group (matches, repeats, misses and npos above the true positives all occur).  Classes of `all_fp` detect far from
    every ground truth, classes of `all_tp` detect each of their ground truths exactly once.  orphan_video: one more video that
    has detections and no ground truth (dropped by the rule)."""
    rs = np.random.RandomState(seed)
    gt_rows, det_rows, by_group = [], [], {}
    for c in range(n_classes):
        for v in range(n_videos):
            ng = int(rs.randint(gt_per_group[0], gt_per_group[1] + 1))
            if v == 0:
                ng = max(ng, 1)
            for _ in range(ng):
                s = float(rs.uniform(0, 100))
                e = s + float(rs.uniform(1, 20))
                by_group.setdefault((c, v), []).append((s, e))
                gt_rows.append((v, c, s, e))
    for c in range(n_classes):
        if c in all_tp:
            for (cc, v), segs in by_group.items():
                if cc == c:
                    det_rows += [(v, c, s, e) for s, e in segs]
            continue
        for _ in range(det_counts[c]):
            v = int(rs.randint(n_videos))
            segs = by_group.get((c, v), [])
            if c in all_fp:
                s = float(rs.uniform(1000, 1100))
                e = s + float(rs.uniform(1, 20))
            elif segs and rs.rand() < 0.5:
                gs, ge = segs[rs.randint(len(segs))]
                s = gs + float(rs.normal(0, 0.25)) * (ge - gs)
                e = s + (ge - gs) * float(rs.uniform(0.6, 1.5))
            else:
                s = float(rs.uniform(0, 100))
                e = s + float(rs.uniform(1, 20))
            det_rows.append((v, c, s, e))
    if orphan_video:
        det_rows += [(n_videos, int(rs.randint(n_classes)), 5.0 + i, 15.0 + i) for i in range(7)]
    return _pack(name, n_classes, _distinct_scores(rs, det_rows), gt_rows, thresholds)


def with_unknown(case):
    """The case plus one video whose only ground truth is of an unknown class (cls = -1): its detections are kept and are
    all false positives.  They get scores between the others', still distinct."""
    det, gt = case['det'], case['gt']
    v = int(max(det['video'].max(initial=-1), gt['video'].max(initial=-1))) + 1
    k = min(case['n_classes'], 3)
    extra = dict(video=np.full(2 * k, v, dtype=np.int32), cls=np.repeat(np.arange(k, dtype=np.int32), 2),
                 seg=np.tile(np.array([[10.0, 20.0], [12.0, 19.0]]), (k, 1)),
                 score=np.float32(0.5) + np.float32(2.0 ** -12) * (1 + np.arange(2 * k)).astype(np.float32))
    assert not np.isin(extra['score'], det['score']).any()
    out = dict(case, name=case['name'] + '+unknown')
    out['det'] = {key: np.concatenate([det[key], extra[key]]) for key in det}
    out['gt'] = dict(video=np.append(gt['video'], np.int32(v)), cls=np.append(gt['cls'], np.int32(-1)),
                     seg=np.concatenate([gt['seg'], [[10.0, 20.0]]]))
    return out


def shared_tiou_case(chain):
    """A detection [10, 20] whose tIoU with the ground truths [10, 25] and [5, 20] is the same 2/3: the lower row is taken.
    chain: a second, lower-scored detection [6, 20] follows, which matches only if [5, 20] is still free -- the host loops
    leave that to the numpy build."""
    gt_rows = [(0, 0, 10.0, 25.0), (0, 0, 5.0, 20.0), (0, 0, 50.0, 60.0)]
    det_rows = [(0, 0, 10.0, 20.0, 0.9), (0, 0, 50.0, 61.0, 0.8), (0, 0, 70.0, 80.0, 0.7)]
    if chain:
        det_rows.append((0, 0, 6.0, 20.0, 0.6))
    return _pack('shared_tiou_chain' if chain else 'shared_tiou', 1, det_rows, gt_rows, [0.5, 0.6, 0.9], host=not chain)


def tie_case():
    """Equal scores inside a class go by table row: a top false positive, then at 0.5 a false positive BEFORE the two true
    positives.  precision 0, 0, 1/3, 2/4 -> envelope 1/2 -> AP = (1/2) (1/2) + (1/2) (1/2) = 1/2; the other order of the tie
    (true positives first) would give 2/3."""
    gt_rows = [(0, 0, 0.0, 10.0), (0, 0, 20.0, 30.0)]
    det_rows = [(0, 0, 100.0, 110.0, 0.5), (0, 0, 0.0, 10.0, 0.5), (0, 0, 20.0, 30.0, 0.5), (0, 0, 40.0, 50.0, 0.9)]
    return _pack('tied_scores', 1, det_rows, gt_rows, [0.5], host=False)


TIE_AP = 0.5


def tied_random_case():
    """random_case with scores quantised to 8 levels: many ties in every class."""
    case = random_case('tied_random', 11, 4, 3, [40, 2 * TILE + 3, 7, 90])
    case['det']['score'] = (np.floor(case['det']['score'] * 8) / 8 + np.float32(0.0625)).astype(np.float32)
    return dict(case, host=False)


def base_cases():
    """The cases without unknown ground truth."""
    return [
        random_case('one_class_one_video', 1, 1, 1, [9], gt_per_group=(3, 3), orphan_video=False),
        random_case('15x6', 2, 15, 6, [int(x) for x in np.random.RandomState(2).randint(0, 120, 15)]),
        random_case('150x3', 3, 150, 3, [int(x) for x in np.random.RandomState(3).randint(0, 30, 150)]),
        # classes 1 and 4 without detections, class 2 all false positives, class 3 all true positives
        random_case('empty_fp_tp', 4, 6, 4, [30, 0, 25, 0, 0, 40], all_fp=(2,), all_tp=(3,)),
        random_case('class_sizes', 5, len(CLASS_SIZES), 5, list(CLASS_SIZES), gt_per_group=(0, 40)),
        random_case('nthr1', 6, 15, 6, [50] * 15, thresholds=THRESHOLD_SETS[1]),
        random_case('nthr10', 7, 15, 6, [50] * 15, thresholds=THRESHOLD_SETS[10]),
        random_case('nthr32', 8, 15, 6, [50] * 15, thresholds=THRESHOLD_SETS[32]),
        shared_tiou_case(chain=False),
    ]


def reference_only_cases():
    """Ties: the host evaluator's result is not determined; ap_reference's is."""
    return [shared_tiou_case(chain=True), tie_case(), tied_random_case()]


def all_cases():
    base = base_cases()
    return base + [with_unknown(c) for c in base] + reference_only_cases()


def npos_max(case):
    """The largest ground-truth count of a class: the npos of the tolerance."""
    cls = case['gt']['cls']
    return int(np.bincount(cls[cls >= 0], minlength=case['n_classes']).max())


def video_name(v):
    return "video_%04d" % v


def write_files(case, directory):
    """The case through the real file layout: ground-truth JSON (subset 'test'; cls -1 as the label 'Unknown'), prediction
    JSON and a THUMOS14-style class index file ('<index> <name>').  -> (gt path, prediction path, class file path)."""
    det, gt, K = case['det'], case['gt'], case['n_classes']
    label = lambda c: "Class%03d" % c if c >= 0 else "Unknown"
    database = {}
    for v, c, seg in zip(gt['video'].tolist(), gt['cls'].tolist(), gt['seg'].tolist()):
        database.setdefault(video_name(v), dict(subset='test', annotations=[]))['annotations'].append(
            dict(label=label(c), segment=seg))
    results = {}
    for v, c, seg, s in zip(det['video'].tolist(), det['cls'].tolist(), det['seg'].tolist(), det['score'].tolist()):
        results.setdefault(video_name(v), []).append(dict(label=label(c), score=s, segment=seg, uncertainty=0.0, actionness=0.0))
    paths = [os.path.join(str(directory), n) for n in ('gt.json', 'pred.json', 'classes.txt')]
    with open(paths[0], 'w') as f:
        json.dump(dict(database=database), f)
    with open(paths[1], 'w') as f:
        json.dump(dict(version='test', results=results, external_data={}), f)
    with open(paths[2], 'w') as f:
        f.write("".join("%d %s\n" % (c + 1, label(c)) for c in range(K)))
    return tuple(paths)


def device_tables(case, device, pieces=1):
    """The case's detections as `pieces` device tables in ops.detection_table's layout, cut at video boundaries where that
    is possible; every table has spare rows past its n, filled with rows that would change the result if they were read."""
    import torch
    det = case['det']
    N = len(det['video'])
    cuts = [0]
    for p in range(1, pieces):
        i = N * p // pieces
        while 0 < i < N and det['video'][i] == det['video'][i - 1]:
            i += 1
        cuts.append(max(i, cuts[-1]))
    cuts.append(N)
    tables = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        n, spare = b - a, 5
        pad = lambda x, fill: np.concatenate([x[a:b], np.full((spare,) + x.shape[1:], fill, dtype=x.dtype)])
        sup = np.zeros((n + spare, 3), dtype=np.float32)
        sup[:n, 0] = det['score'][a:b]
        sup[n:, 0] = 2.0                    # a spare row would outrank everything
        tables.append(dict(video=torch.from_numpy(pad(det['video'], 0)).to(device),
                           cls=torch.from_numpy(pad(det['cls'], 0)).to(device),
                           seg=torch.from_numpy(pad(det['seg'], 1.0)).to(device), sup=torch.from_numpy(sup).to(device),
                           n=torch.tensor(n, dtype=torch.int32, device=device)))
    return tables


def ground_truth(case):
    """The case's ground truth as a table_ap.GroundTruth, without a file; every video of the case is numbered."""
    from opental_amd.evaluation.table_ap import GroundTruth
    nvid = int(max(case['det']['video'].max(initial=-1), case['gt']['video'].max(initial=-1))) + 1
    return GroundTruth(case['gt']['video'], case['gt']['cls'], case['gt']['seg'], case['n_classes'],
                       {video_name(v): v for v in range(nvid)})
