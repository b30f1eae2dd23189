"""Shared inputs of test_table_open_cpu.py / test_table_open_gpu.py: hand-made results of the split pass -- codes, the
positions' table rows, the tables' known / cls columns and the ground truths' classes, the arguments of
table_open.codes_reference / codes_to_curves -- at the edges of the curve kernel's wave (64) and workgroup tile, and seeded
(det, gt) column sets for the whole path.  TILE is the kernel's tile, from the one constant the wrapper exports.

A case is built from its threshold-0 foreground in list order (ascending known): one (known, unknown, correct) triple per
entry.  Entry j is a detection at an odd group-sorted position, between background rows (codes -1 and -2 in turn); positions
map to table rows by a seeded permutation and the entries take seeded ground-truth rows, so the scatter and the sorts have
something to do.  Threshold t > 0 leaves out the first t % 3 entries and gives their ground truths to nobody.  Known-ness
values are multiples of 2^-10 below 1: `1 - known` is exact."""
import json
import os

import numpy as np

from opental_amd.common.ops import AP_TILE as TILE
from table_ap_cases import video_name

WAVE = 64
SIZES = (0, 1, 2, 3, WAVE - 1, WAVE, WAVE + 1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1)
N_CLASSES = 4


def _kinds(rs, n, p_unknown=0.4, p_correct=0.7):
    unknown = rs.rand(n) < p_unknown
    return unknown, (rs.rand(n) < p_correct) & ~unknown


def build(name, known, unknown, correct, nthr=1, ood_threshold=None, seed=0, gap_after=None):
    """known (n) ascending fp64, unknown / correct (n) bool: the threshold-0 list -> a case."""
    rs = np.random.RandomState(1000 + seed)
    known, unknown, correct = np.asarray(known, dtype=np.float64), np.asarray(unknown, bool), np.asarray(correct, bool)
    n = len(known)
    assert (np.diff(known) >= 0).all() and not (unknown & correct).any()
    # group-sorted positions: background, entry 0, background, entry 1, ... with an optional stretch of TILE background rows
    kinds = []
    for j in range(n):
        kinds += [-1, j]
        if gap_after is not None and j == gap_after:
            kinds += [-1] * TILE
    kinds += [-1, -1, -1]
    N, M = len(kinds), n + 3
    entry_pos = np.array([p for p, k in enumerate(kinds) if k >= 0], dtype=np.int64)
    row = rs.permutation(N)                                     # position -> table row
    gt_of = rs.permutation(M)[:n]                               # entry -> ground-truth row
    gt_cls = rs.randint(0, N_CLASSES, M).astype(np.int32)
    gt_cls[gt_of[unknown]] = -1
    tab_known = (rs.randint(1, 1024, N) / 1024.0)               # the background rows: values that must not be read
    tab_cls = rs.randint(0, N_CLASSES, N).astype(np.int64)
    # equal known-ness goes by table row: hand the entries of a tie group their rows in ascending order
    entry_rows = row[entry_pos]
    for v in np.unique(known):
        idx = np.nonzero(known == v)[0]
        entry_rows[idx] = np.sort(entry_rows[idx])
    row[entry_pos] = entry_rows
    tab_known[entry_rows] = known
    g = gt_cls[gt_of]
    tab_cls[entry_rows] = np.where(correct, g, (np.maximum(g, 0) + 1) % N_CLASSES)
    codes = np.empty((nthr, N), dtype=np.int32)
    background = np.array([-1 - (p % 2) for p in range(N)], dtype=np.int32)
    for t in range(nthr):
        codes[t] = background
        first = t % 3 if n > 3 else 0
        codes[t, entry_pos[first:]] = gt_of[first:]
    return dict(name=name, codes=codes, row=row, known=tab_known, cls=tab_cls, gt_cls=gt_cls, ood_threshold=ood_threshold,
                n=n, list=(known, unknown, correct))


def _tie_free(n):
    return (1.0 + np.arange(n)) / 1024.0


def size_case(n, seed):
    rs = np.random.RandomState(seed)
    unknown, correct = _kinds(rs, n)
    return build('n%d' % n, _tie_free(n), unknown, correct, seed=seed)


def pairs20():
    """Twenty tied (unknown, known) pairs: tpr_j = fpr_j = j / 20; drop_intermediate keeps j = 1 and j = 20: FAR@95 = 1.0."""
    known = np.repeat((1.0 + np.arange(20)) / 32.0, 2)
    unknown = np.tile([True, False], 20)
    return build('pairs20', known, unknown, ~unknown, seed=40)


def kernel_cases():
    """Every case of the curve kernel."""
    cases = [size_case(n, i) for i, n in enumerate(SIZES)]
    rs = np.random.RandomState(77)
    n = 2 * TILE + 1
    unknown, correct = _kinds(rs, n)
    cases.append(build('all_equal', np.full(n, 0.5), unknown, correct, seed=20))
    known = _tie_free(n)
    known[60:71] = known[60]
    cases.append(build('tie_over_wave_edge', known, unknown, correct, seed=21))
    known = _tie_free(n)
    known[250:263] = known[250]
    cases.append(build('tie_over_chunk_edge', known, unknown, correct, seed=22))
    cases.append(pairs20())
    none = np.zeros(n, dtype=bool)
    cases.append(build('only_known', _tie_free(n), none, correct | (rs.rand(n) < 0.3), seed=23))
    cases.append(build('only_unknown', _tie_free(n), ~none, none, seed=24))
    # the last 70 entries are known matches with distinct scores: equal fps steps on tps = P, collinear up to the last entry
    tail = unknown.copy()
    tail[-70:] = False
    cases.append(build('collinear_tail', _tie_free(n), tail, correct & ~tail, seed=25))
    # runs of equal-step points in the middle, across both edges: unknown, known alternating
    alt = (np.arange(n) % 2).astype(bool)
    cases.append(build('alternating', _tie_free(n), alt, ~alt, seed=26))
    cases.append(build('nthr5', _tie_free(WAVE + 1), unknown[:WAVE + 1], correct[:WAVE + 1], nthr=5, seed=27))
    cases.append(build('nthr32', _tie_free(TILE + 1), unknown[:TILE + 1], correct[:TILE + 1], nthr=32, seed=28))
    cases.append(build('gap', _tie_free(n), unknown, correct, seed=29, gap_after=100))
    # relabelling: ood < 0.75 <=> known > 0.25 (entries 256 ..): some correct rows become "unknown" predictions
    assert correct[300:].any() and correct[:200].any()
    cases.append(build('relabel', _tie_free(n), unknown, correct, ood_threshold=0.75, seed=30))
    cases.append(build('relabel_ties', np.floor(_tie_free(n) * 16) / 16 + 0.03125, unknown, correct, nthr=5, ood_threshold=0.8,
                       seed=31))
    return cases


def expected_flags(case, t=0):
    """The (correct, unknown) flags of threshold t's list after the relabelling, in list order."""
    known, unknown, correct = case['list']
    first = t % 3 if case['n'] > 3 else 0
    if case['ood_threshold'] is not None:
        correct = correct & ~((1.0 - known) < case['ood_threshold'])
    return known[first:], unknown[first:], correct[first:]


# ----------------------------------------------------------------------------------------------- (det, gt) column sets
def table_case(name, seed, n_videos=3, gt_per_video=30, det_per_video=80, thresholds=(0.3, 0.5, 0.7), orphan=True, ties=False):
    """Random segments in the columns of open_reference: every video gets gt_per_video ground truths, about 40 % of them of an
    unknown class, and det_per_video detections in (video, class) order, about half of them jittered copies of a ground truth;
    known-ness values are distinct multiples of 2^-20 (`ties`: quantised to 16 levels).  orphan: one more video with
    detections and no ground truth."""
    rs = np.random.RandomState(seed)
    gt_rows, det_rows = [], []
    for v in range(n_videos):
        segs = []
        for _ in range(gt_per_video):
            s = float(rs.uniform(0, 300))
            e = s + float(rs.uniform(2, 20))
            c = -1 if rs.rand() < 0.4 else int(rs.randint(N_CLASSES))
            segs.append((s, e, c))
            gt_rows.append((v, c, s, e))
        for _ in range(det_per_video):
            if rs.rand() < 0.5:
                gs, ge, gc = segs[rs.randint(len(segs))]
                s = gs + float(rs.normal(0, 0.15)) * (ge - gs)
                e = s + (ge - gs) * float(rs.uniform(0.7, 1.3))
                c = gc if gc >= 0 and rs.rand() < 0.7 else int(rs.randint(N_CLASSES))
            else:
                s = float(rs.uniform(0, 300))
                e = s + float(rs.uniform(2, 20))
                c = int(rs.randint(N_CLASSES))
            det_rows.append((v, c, s, e))
    if orphan:
        det_rows += [(n_videos, int(rs.randint(N_CLASSES)), 5.0 + i, 15.0 + i) for i in range(7)]
    det_rows = sorted(det_rows, key=lambda r: (r[0], r[1]))
    n = len(det_rows)
    known = (1.0 + rs.permutation(n)) / 2.0 ** 20 * (2 ** 20 // (n + 1))
    if ties:
        known = np.floor(known * 16) / 16 + 0.03125
    det = dict(video=np.array([r[0] for r in det_rows], dtype=np.int32), cls=np.array([r[1] for r in det_rows], dtype=np.int32),
               seg=np.array([r[2:4] for r in det_rows], dtype=np.float64).reshape(-1, 2), known=known.astype(np.float64))
    gt = dict(video=np.array([r[0] for r in gt_rows], dtype=np.int32), cls=np.array([r[1] for r in gt_rows], dtype=np.int32),
              seg=np.array([r[2:4] for r in gt_rows], dtype=np.float64).reshape(-1, 2))
    return dict(name=name, det=det, gt=gt, thresholds=list(thresholds), n_classes=N_CLASSES)


def host_cases():
    """Tie-free column sets whose host result is determined."""
    return [table_case('3x30', 1), table_case('1x60', 2, n_videos=1, gt_per_video=60, det_per_video=200, orphan=False),
            table_case('5thr', 3, thresholds=(0.1, 0.3, 0.5, 0.7, 0.9))]


def write_files(case, directory):
    """The case through the real file layout: ground-truth JSON (subset 'test'; cls -1 as the label 'Unknown'), a prediction
    JSON built by proposals_from_table from the case's table (uncertainty = 1 - known, exact) and a THUMOS14-style class file.
    -> (gt path, prediction path, class file path)."""
    import torch
    from opental_amd.common.det_table import proposals_from_table
    det, gt, K = case['det'], case['gt'], case['n_classes']
    label = lambda c: "Class%03d" % c if c >= 0 else "Unknown"
    nvid = int(max(det['video'].max(initial=-1), gt['video'].max(initial=-1))) + 1
    database = {}
    for v, c, seg in zip(gt['video'].tolist(), gt['cls'].tolist(), gt['seg'].tolist()):
        database.setdefault(video_name(v), dict(subset='test', annotations=[]))['annotations'].append(
            dict(label=label(c), segment=seg))
    n = len(det['video'])
    key = det['video'].astype(np.int64) * K + det['cls']
    assert (np.diff(key) >= 0).all()
    sup = np.zeros((n, 3), dtype=np.float32)
    sup[:, 0] = 0.5
    sup[:, 1] = (1.0 - det['known']).astype(np.float32)
    assert np.array_equal(sup[:, 1].astype(np.float64), 1.0 - det['known'])     # multiples of 2^-20: exact in fp32
    table = dict(video=torch.from_numpy(det['video']), cls=torch.from_numpy(det['cls']), seg=torch.from_numpy(det['seg']),
                 sup=torch.from_numpy(sup), known=torch.from_numpy(det['known']), n=n,
                 list_start=torch.from_numpy(np.searchsorted(key, np.arange(nvid * K + 1)).astype(np.int32)))
    names = [video_name(v) for v in range(nvid)]
    results = proposals_from_table(table, names, {c + 1: label(c) for c in range(K)})
    paths = [os.path.join(str(directory), f) for f in ('gt.json', 'pred.json', 'classes.txt')]
    with open(paths[0], 'w') as f:
        json.dump(dict(database=database), f)
    with open(paths[1], 'w') as f:
        json.dump(dict(version='test', results=results, external_data={}), f)
    with open(paths[2], 'w') as f:
        f.write("".join("%d %s\n" % (c + 1, label(c)) for c in range(K)))
    return tuple(paths)
