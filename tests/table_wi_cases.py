"""Shared inputs of test_table_wi_cpu.py / test_table_wi_gpu.py: seeded results of the labelled matching -- codes, the
positions' labels, the ground truths' labels and the two totals, the arguments of table_wi.codes_reference and
ops.wilderness_impact -- at the edges of the kernel's tile, and seeded (det, gt) column sets for the whole path, with the
files the host evaluator reads.  TILE is the kernel's tile, from the one constant the wrapper exports.

A kernel case draws, per position, a code (a ground-truth row, -1 or -2) and a label that agrees with the matched ground
truth's about half the time; `u_rows` are forced to be tp_u2u (label 0 on an unknown ground truth).  n_unknown is the largest
tp_u2u count of a threshold plus 2 (the recall ratio stays below 1) unless `found_all` asks for exactly that count."""
import json
import os

import numpy as np

from opental_amd.common.ops import AP_TILE as TILE

SIZES = (0, 1, TILE - 1, TILE, TILE + 1, 3 * TILE + 7)


def kernel_case(name, N, K, nthr=1, seed=0, u_rows=(), last_tile_class=False, all_unknown=False, found_all=False):
    rs = np.random.RandomState(2000 + seed)
    M = N // 2 + 4
    gt_label = rs.randint(1, K + 1, M).astype(np.int32)
    gt_label[rs.rand(M) < 0.4] = 0
    gt_label[0], gt_label[1] = 0, 1                             # both kinds exist
    unknown_rows = np.nonzero(gt_label == 0)[0]
    codes = np.empty((nthr, N), dtype=np.int32)
    for t in range(nthr):
        kind = rs.rand(N)
        codes[t] = np.where(kind < 0.55, rs.randint(0, M, N), np.where(kind < 0.85, -1, -2))
    pred_label = rs.randint(0, K + 1, N).astype(np.int32)
    agree = rs.rand(N) < 0.5
    matched = gt_label[np.maximum(codes[0], 0)]
    pred_label = np.where(agree & (codes[0] >= 0), matched, pred_label).astype(np.int32)
    if last_tile_class:                                         # label K only in the last tile, and there for sure
        start = (N - 1) // TILE * TILE
        pred_label[:start][pred_label[:start] == K] = 1 if K > 1 else 0
        pred_label[start:][::3] = K
        codes[:, start:][:, ::6] = -1                           # some of them background: fp_bg2k of that class
    if all_unknown:
        pred_label[:] = 0
    for r in u_rows:
        pred_label[r] = 0
        codes[:, r] = unknown_rows[r % len(unknown_rows)]
    u_counts = [int(((codes[t] >= 0) & (pred_label == 0) & (gt_label[np.maximum(codes[t], 0)] == 0)).sum()) for t in range(nthr)]
    n_unknown = max(u_counts, default=0) + (0 if found_all else 2)
    return dict(name=name, codes=codes, pred_label=pred_label, gt_label=gt_label, n_known=int((gt_label > 0).sum()) + 5,
                n_unknown=n_unknown, K=K, m=max(u_counts, default=0) + 1, u_counts=u_counts)


def kernel_cases():
    """Every case of the WI kernel: the tile's edges, K in {1, 15, 20}, nthr in {1, 5, 32} and the placed rows."""
    big = 3 * TILE + 7
    cases = [kernel_case('n%d' % n, n, 15, seed=i) for i, n in enumerate(SIZES)]
    cases += [kernel_case('k1', big, 1, seed=10), kernel_case('k20_nthr5', big, 20, nthr=5, seed=11),
              kernel_case('nthr32', TILE + 1, 15, nthr=32, seed=12),
              kernel_case('u_first_row', big, 15, seed=13, u_rows=(0,)),
              kernel_case('u_last_row', big, 15, seed=14, u_rows=(big - 1,)),
              kernel_case('u_on_tile_edges', big, 15, nthr=5, seed=15, u_rows=(TILE - 1, TILE, 2 * TILE, 3 * TILE)),
              kernel_case('class_in_last_tile', big, 20, seed=16, last_tile_class=True),
              kernel_case('all_predicted_unknown', big, 15, nthr=5, seed=17, all_unknown=True),
              kernel_case('found_all', 2 * TILE, 15, seed=18, u_rows=(5, TILE + 3), found_all=True)]
    return cases


def polluted(case, seed=0):
    """The case with out-of-range codes and labels written over rows that have no outcome (code -2), and with two further
    ground-truth rows of out-of-range labels that a few such rows point to: the result must not change."""
    rs = np.random.RandomState(3000 + seed)
    codes, pred_label, gt_label = case['codes'].copy(), case['pred_label'].copy(), case['gt_label'].copy()
    K, M = case['K'], len(gt_label)
    gt_label = np.concatenate((gt_label, np.array([K + 1, -1], dtype=np.int32)))
    free = np.nonzero((codes == -2).all(axis=0))[0]
    assert len(free) >= 8
    picks = rs.permutation(free)[:8]
    big = np.iinfo(np.int32)
    for r, bad in zip(picks[:4], (M + 2, -3, big.max, big.min)):
        codes[:, r] = bad
    for r, bad in zip(picks[4:6], (M, M + 1)):                  # in-range codes onto the out-of-range ground-truth labels
        codes[:, r] = bad
    for r, bad in zip(picks[6:8], (K + 1, -1)):                 # out-of-range labels of the detection
        codes[:, r] = -1                                        # ... on a row that would otherwise be a background one
        pred_label[r] = bad
    return dict(case, name=case['name'] + '_polluted', codes=codes, pred_label=pred_label, gt_label=gt_label)


# ----------------------------------------------------------------------------------------------- (det, gt) column sets
def _tiou(a, b):
    inter = np.clip(np.minimum(a[:, None, 1], b[None, :, 1]) - np.maximum(a[:, None, 0], b[None, :, 0]), 0, None)
    union = (a[:, 1] - a[:, 0])[:, None] + (b[:, 1] - b[:, 0])[None, :] - inter
    return inter / union


def table_case(name, seed, n_videos=3, gt_per_video=24, det_per_video=70, thresholds=(0.3, 0.5, 0.7), n_classes=4, orphan=False,
               outside=False, ties=False, names=None):
    """Random segments in the columns of wi_reference: every video gets gt_per_video ground truths, about 40 % of them of an
    unknown class, and det_per_video detections in (video, class) order, about 60 % of them jittered copies of a ground truth;
    known-ness values are distinct multiples of 2^-20.  A detection is drawn again until none of its tIoUs with the video's
    ground truths lies within 1e-3 of a threshold, so no comparison turns on a rounding.  orphan: one more video with detections and
    no ground truth; outside: a few detections of class n_classes (outside the index); ties: every third ground truth is
    duplicated under another label (equal tIoU: the lowest row wins).  names: the videos' names in number order."""
    rs = np.random.RandomState(seed)
    thr = np.asarray(thresholds)
    gt_rows, det_rows = [], []
    for v in range(n_videos):
        segs, dets = [], []
        for i in range(gt_per_video):
            s = float(rs.uniform(0, 300))
            e = s + float(rs.uniform(2, 20))
            c = -1 if rs.rand() < 0.4 else int(rs.randint(n_classes))
            segs.append((s, e, c))
            if ties and i % 3 == 0:
                segs.append((s, e, -1 if c >= 0 else int(rs.randint(n_classes))))
        gt_seg = np.array([g[:2] for g in segs])
        while len(dets) < det_per_video:
            if rs.rand() < 0.6:
                gs, ge, gc = segs[rs.randint(len(segs))]
                s = gs + float(rs.normal(0, 0.12)) * (ge - gs)
                e = s + (ge - gs) * float(rs.uniform(0.75, 1.25))
                c = gc if gc >= 0 and rs.rand() < 0.7 else int(rs.randint(n_classes))
            else:
                s = float(rs.uniform(0, 300))
                e = s + float(rs.uniform(2, 20))
                c = int(rs.randint(n_classes))
            t = _tiou(np.array([[s, e]]), gt_seg)
            if np.abs(t[:, :, None] - thr[None, None, :]).min() > 1e-3:        # drawn again otherwise
                dets.append((s, e, c))
        gt_rows += [(v, c, s, e) for s, e, c in segs]
        det_rows += [(v, c, s, e) for s, e, c in dets]
    if outside:
        det_rows += [(0, n_classes, 5.0 + i, 15.0 + i) for i in range(3)]
    if orphan:
        det_rows += [(n_videos, int(rs.randint(n_classes)), 5.0 + i, 15.0 + i) for i in range(7)]
    det_rows = sorted(det_rows, key=lambda r: (r[0], r[1]))
    n = len(det_rows)
    known = (1.0 + rs.permutation(n)) / 2.0 ** 20 * (2 ** 20 // (n + 1))
    det = dict(video=np.array([r[0] for r in det_rows], dtype=np.int32), cls=np.array([r[1] for r in det_rows], dtype=np.int32),
               seg=np.array([r[2:4] for r in det_rows], dtype=np.float64).reshape(-1, 2), known=known.astype(np.float64))
    gt = dict(video=np.array([r[0] for r in gt_rows], dtype=np.int32), cls=np.array([r[1] for r in gt_rows], dtype=np.int32),
              seg=np.array([r[2:4] for r in gt_rows], dtype=np.float64).reshape(-1, 2))
    nvid = n_videos + (1 if orphan else 0)
    names = list(names) if names is not None else ["video_%04d" % v for v in range(nvid)]
    assert len(names) == nvid
    return dict(name=name, det=det, gt=gt, thresholds=list(thresholds), n_classes=n_classes, names=names, ood_threshold=0.4,
                m=int((gt['cls'] < 0).sum()) + 1)


def rank_of(case):
    """The rank of each video number of the case in ascending-name order."""
    from opental_amd.evaluation.table_wi import video_rank
    return video_rank({n: v for v, n in enumerate(case['names'])})


def host_cases():
    return [table_case('3x24', 1), table_case('orphan', 2, orphan=True), table_case('outside_class', 3, outside=True),
            table_case('tied_tiou', 4, ties=True, thresholds=(0.1, 0.3, 0.5, 0.7, 0.9)),
            table_case('names_b_a_c', 5, names=['b', 'a', 'c']),
            table_case('1x60', 6, n_videos=1, gt_per_video=60, det_per_video=300)]


def write_files(case, directory):
    """The case through the real file layout: ground-truth JSON (subset 'test'; cls -1 as the label 'Unknown'), a prediction
    JSON (videos in number order, a video's detections in table row order; uncertainty = 1 - known, which the evaluator reads
    back as the same fp64) and a THUMOS14-style class file.  -> (gt path, prediction path, class file path)."""
    det, gt, K, names = case['det'], case['gt'], case['n_classes'], case['names']
    label = lambda c: "Unknown" if c < 0 else "Outside" if c >= K else "Class%03d" % c
    database, results = {}, {}
    for v, c, seg in zip(gt['video'].tolist(), gt['cls'].tolist(), gt['seg'].tolist()):
        database.setdefault(names[v], dict(subset='test', annotations=[]))['annotations'].append(dict(label=label(c), segment=seg))
    for name in names:
        results[name] = []
    for v, c, seg, k in zip(det['video'].tolist(), det['cls'].tolist(), det['seg'].tolist(), det['known'].tolist()):
        results[names[v]].append(dict(label=label(c), score=0.5, segment=seg, uncertainty=1.0 - k, actionness=0.0))
    paths = [os.path.join(str(directory), f) for f in ('gt.json', 'pred.json', 'classes.txt')]
    with open(paths[0], 'w') as f:
        json.dump(dict(database=database), f)
    with open(paths[1], 'w') as f:
        json.dump(dict(version='test', results=results, external_data={}), f)
    with open(paths[2], 'w') as f:
        f.write("".join("%d %s\n" % (c + 1, label(c)) for c in range(K)))
    return tuple(paths)
