"""The detections of a batch of videos as one table instead of one dict per detection.

The inference drivers turn the Soft-NMS output (rows (V, K, top_k, cols), counts (V, K); common.detect.softnms_classes) into
proposal dicts by walking every row in Python (anet.test.get_video_prediction, common.detect.get_video_detections), and the
open-set threshold (common.detect.ood_threshold) walks all the dicts again.  This module states that walk once as a rule over
arrays:

  * `table_reference` -- the rule in plain numpy loops: the oracle of otal_detection_table (csrc/dettable.hip) and the form
    that serves host tensors;
  * `detection_table` -- the table of device tensors through the kernel (ops.detection_table), of host tensors through
    `table_reference`;
  * `proposals_from_table` -- the proposal dicts of the drivers, from a table, for the callers that still want them;
  * `threshold_from_scores` -- the known / unknown operating point from the table's known-ness column.

A table is a dict: video, cls (0-based) int32 (N); seg fp64 (N, 2), clipped; sup fp32 (N, 3) = score, uncertainty,
actionness (0.0 for a column the rows do not carry); known fp64 (N) = 1 - the out-of-distribution score; list_start int32
(V*K + 1), the exclusive prefix of the valid rows per (video, class); n = N.  Rows are in (video, class, row) order, the order
of the host loops.  The device table is allocated at the upper bound V*K*top_k and n is a device scalar: only the first n
rows mean anything."""
import numpy as np
import torch

from .detect import OOD_SCORES

SCORINGS = tuple(OOD_SCORES)        # the kernel's `scoring` argument is the index into this tuple


def table_reference(rows, counts, durations=None, drop_empty=False, scoring='uncertainty'):
    """The rule, row by row.  rows (V, K, top_k, cols) float32 with cols 3..5, counts (V, K), durations (V) seconds or None.
    Row (v, c, i) is kept when i < counts[v, c] and its score is > 0 (a NaN score is not); with `durations` or `drop_empty`
    the segment is clipped as the drivers clip it (start to >= 0, end to <= the duration when there is one) and the row is
    dropped when end <= start.  Rows at and past counts[v, c] are never looked at."""
    rows, counts = np.asarray(rows, dtype=np.float32), np.asarray(counts)
    V, K, top_k, cols = rows.shape
    if not 3 <= cols <= 5:
        raise ValueError("rows have 3 to 5 columns, got %d" % cols)
    ood = OOD_SCORES[scoring]
    clip = durations is not None or drop_empty
    video, cls, seg, sup, known, list_start = [], [], [], [], [], []
    for v in range(V):
        for c in range(K):
            list_start.append(len(video))
            for i in range(min(max(int(counts[v, c]), 0), top_k)):
                r = rows[v, c, i]
                if not r[2] > 0:
                    continue
                start, end = float(r[0]), float(r[1])
                if clip:
                    start = max(0.0, start)
                    if durations is not None:
                        end = min(float(durations[v]), end)
                    if end <= start:
                        continue
                score = float(r[2])
                unct = float(r[3]) if cols > 3 else 0.0
                actn = float(r[4]) if cols > 4 else 0.0
                video.append(v)
                cls.append(c)
                seg.append((start, end))
                sup.append((r[2], r[3] if cols > 3 else 0.0, r[4] if cols > 4 else 0.0))
                known.append(1 - ood({'score': score, 'uncertainty': unct, 'actionness': actn}))
    list_start.append(len(video))
    return dict(video=np.array(video, dtype=np.int32), cls=np.array(cls, dtype=np.int32),
                seg=np.array(seg, dtype=np.float64).reshape(-1, 2), sup=np.array(sup, dtype=np.float32).reshape(-1, 3),
                known=np.array(known, dtype=np.float64), list_start=np.array(list_start, dtype=np.int32), n=len(video))


def detection_table(rows, counts, durations=None, drop_empty=False, scoring='uncertainty'):
    """The table of the Soft-NMS output: device tensors go through otal_detection_table, host tensors through
    `table_reference` (returned as host tensors of exactly n rows, n a 0-dim tensor)."""
    if rows.is_cuda:
        from . import ops
        return ops.detection_table(rows, counts, durations, drop_empty, scoring)
    ref = table_reference(rows.numpy(), counts.numpy(), None if durations is None else np.asarray(durations, dtype=np.float64),
                          drop_empty, scoring)
    return {k: torch.as_tensor(v) for k, v in ref.items()}


def _host(a, n):
    return (a[:n].cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)[:n])


def proposals_from_table(table, names, idx_to_class=None):
    """{names[v]: [proposal dict, ...]} of a table over len(names) videos: what anet.test.get_video_prediction /
    common.detect.get_video_detections build from the same rows (a clipped start is 0.0 where those give the int 0).
    The columns come to the host once and become Python numbers by tolist()."""
    n = int(table['n'])
    starts = _host(table['list_start'], None).tolist()
    V = len(names)
    if V == 0 or (len(starts) - 1) % V:
        raise ValueError("list_start does not hold a whole number of classes for %d videos" % V)
    K = (len(starts) - 1) // V
    label = [idx_to_class[c + 1] if idx_to_class is not None else c + 1 for c in range(K)]
    cls = _host(table['cls'], n).tolist()
    seg = _host(table['seg'], n).tolist()
    sup = _host(table['sup'], n).astype(np.float64).tolist()        # float(np.float32): the exact widening
    flat = [{'label': label[c], 'score': s[0], 'segment': sg, 'uncertainty': s[1], 'actionness': s[2]}
            for c, sg, s in zip(cls, seg, sup)]
    return {name: flat[starts[v * K]:starts[(v + 1) * K]] for v, name in enumerate(names)}


def threshold_index(n):
    """The position, in ascending order, of the known-ness score that 95 % of n detections exceed (threshold.py:144-147)."""
    return n - int(n * 0.95) - 1


def threshold_from_scores(scores):
    """common.detect.ood_threshold over a column of known-ness scores (fp64; a device or host tensor, or an array)."""
    scores = torch.as_tensor(scores, dtype=torch.float64).reshape(-1)
    n = scores.numel()
    if n == 0:
        raise ValueError("no detections to threshold")
    return float(torch.sort(scores).values[threshold_index(n)])
