"""CPU: the detection-table rule of opental_amd/common/det_table.py (table_reference, proposals_from_table,
threshold_from_scores) against the host loops it restates (anet.test.get_video_prediction,
thumos14.test.get_video_detections, thumos14.test.ood_threshold), the reference's compute_threshold pinned in
tests/golden/anet_threshold.npz, the selection index, and otal_detection_table's argument codes."""
import ctypes
import os

import numpy as np
import pytest
import torch

from det_table_cases import SCORINGS, make_case

V, K, TOP_K = 3, 5, 7
NAMES = ['vid_a', 'vid_b', 'vid_c']
IDX_TO_CLASS = {c + 1: 'class_%d' % c for c in range(K)}


def _case(cols):
    rows, counts, durations = make_case(V, K, TOP_K, cols, seed=cols)
    assert counts.min() == 0 and counts.max() == TOP_K
    assert (rows[..., 2] == 1e6).any() and np.isnan(rows[..., 2]).any() and (rows[..., 2] == 0).any() and (rows[..., 2] == -1).any()
    assert (rows[..., 0] < 0).any() and (rows[..., 0] == rows[..., 1]).any()
    assert (rows[..., 1] > durations[:, None, None]).any() and (rows[..., 0] > durations[:, None, None]).any()
    return rows, counts, durations


def _loops(rows, counts, fn):
    return {NAMES[v]: fn(torch.from_numpy(rows[v]), torch.from_numpy(counts[v]), v) for v in range(V)}


@pytest.mark.parametrize("cols", [3, 4, 5])
def test_table_equals_the_host_loops(cols):
    from opental_amd.anet.test import get_video_prediction
    from opental_amd.common.det_table import proposals_from_table, table_reference
    from opental_amd.thumos14.test import get_video_detections
    rows, counts, durations = _case(cols)
    variants = {
        'anet': (dict(durations=durations), lambda r, c, v: get_video_prediction(r, c, float(durations[v]), IDX_TO_CLASS)),
        'plain': (dict(), lambda r, c, v: get_video_detections(r, c, IDX_TO_CLASS)),
        'duration': (dict(durations=durations), lambda r, c, v: get_video_detections(r, c, IDX_TO_CLASS, duration=float(durations[v]))),
        'drop_empty': (dict(drop_empty=True), lambda r, c, v: get_video_detections(r, c, IDX_TO_CLASS, drop_empty=True)),
    }
    for name, (kw, fn) in variants.items():
        table = table_reference(rows, counts, **kw)
        share = table['n'] / float(V * K * TOP_K)
        assert share >= 0.4, (name, share)          # a test that passes on an empty table shows nothing
        want = _loops(rows, counts, fn)
        got = proposals_from_table(table, NAMES, IDX_TO_CLASS)
        assert got == want, name
        assert sum(len(p) for p in got.values()) == table['n'] == int(table['list_start'][-1])
        # the columns say the same as the dicts
        flat = [p for n in NAMES for p in want[n]]
        assert table['seg'].tolist() == [p['segment'] for p in flat]
        assert table['sup'].astype(np.float64).tolist() == [[p['score'], p['uncertainty'], p['actionness']] for p in flat]
        assert [IDX_TO_CLASS[c + 1] for c in table['cls'].tolist()] == [p['label'] for p in flat]
        assert table['video'].tolist() == [v for v, n in enumerate(NAMES) for _ in want[n]]
    # without class names the label is the 1-based class index, as in the loops
    got = proposals_from_table(table_reference(rows, counts), NAMES)
    assert got == _loops(rows, counts, lambda r, c, v: get_video_detections(r, c))
    # the plain table keeps what the clipping variants drop
    assert table_reference(rows, counts)['n'] > table_reference(rows, counts, drop_empty=True)['n'] \
        > table_reference(rows, counts, durations=durations)['n']


@pytest.mark.parametrize("scoring", SCORINGS)
def test_threshold_equals_ood_threshold_bit_for_bit(scoring):
    from opental_amd.anet.test import get_video_prediction
    from opental_amd.common.det_table import SCORINGS as ORDER, table_reference, threshold_from_scores
    from opental_amd.thumos14.test import OOD_SCORES, ood_threshold
    assert ORDER == SCORINGS == tuple(OOD_SCORES)
    rows, counts, durations = _case(5)
    dicts = _loops(rows, counts, lambda r, c, v: get_video_prediction(r, c, float(durations[v])))
    table = table_reference(rows, counts, durations, scoring=scoring)
    assert table['n'] >= 0.4 * V * K * TOP_K
    assert table['known'].tolist() == [1 - OOD_SCORES[scoring](p) for n in NAMES for p in dicts[n]]
    assert threshold_from_scores(table['known']) == ood_threshold(dicts, scoring)
    assert threshold_from_scores(torch.from_numpy(table['known'])) == ood_threshold(dicts, scoring)


def test_threshold_equals_the_reference_compute_threshold(golden_dir):
    """tests/golden/anet_threshold.npz (tools/pin_anet_threshold.py): the reference's compute_threshold on synthetic dicts.
    Its 'confidence' branch takes the score itself where the table holds 1 - (1 - score); for float32 scores >= 2^-29 both
    subtractions are exact in fp64, so the two agree bit for bit."""
    from opental_amd.common.det_table import table_reference, threshold_from_scores
    fx = np.load(os.path.join(golden_dir, "anet_threshold.npz"))
    scorings = [str(s) for s in fx["scorings"]]
    assert scorings == ['uncertainty', 'confidence', 'uncertainty_actionness']
    for n in (1, 20, 137, 1000):
        video, sup, want = fx[f"n{n}_video"], fx[f"n{n}_sup"], fx[f"n{n}_threshold"]
        assert sup.dtype == np.float32 and sup.shape == (n, 3)
        # the detections as Soft-NMS rows: video v's detections are the rows of its one class
        per_video = np.bincount(video, minlength=3)
        rows = np.zeros((3, 1, int(per_video.max()), 5), dtype=np.float32)
        rows[..., 1] = 1.0
        for v in range(3):
            rows[v, 0, :per_video[v], 2:] = sup[video == v]
        for k, scoring in enumerate(scorings):
            table = table_reference(rows, per_video.reshape(3, 1), scoring=scoring)
            assert table['n'] == n
            assert threshold_from_scores(table['known']) == want[k], (n, scoring)


@pytest.mark.parametrize("n,index", [(1, 0), (19, 0), (20, 0), (21, 1), (10001, 500)])
def test_selection_index(n, index):
    from opental_amd.common.det_table import threshold_from_scores, threshold_index
    assert threshold_index(n) == index
    scores = np.random.RandomState(n).permutation(n).astype(np.float64) / 7.0
    assert threshold_from_scores(scores) == index / 7.0 == float(np.sort(scores)[n - int(n * 0.95) - 1])


def test_no_detections_is_an_error():
    from opental_amd.common.det_table import table_reference, threshold_from_scores
    rows, counts, durations = make_case(2, 2, 3, 5, counts=0)
    table = table_reference(rows, counts, durations)
    assert table['n'] == 0 and table['list_start'].tolist() == [0] * 5
    with pytest.raises(ValueError, match="no detections to threshold"):
        threshold_from_scores(table['known'])


def test_host_tensors_take_the_reference_path():
    from opental_amd.common.det_table import detection_table, table_reference
    rows, counts, durations = _case(5)
    got = detection_table(torch.from_numpy(rows), torch.from_numpy(counts), durations.tolist(), scoring='half_au')
    want = table_reference(rows, counts, durations, scoring='half_au')
    assert int(got['n']) == want['n']
    for k in ('video', 'cls', 'seg', 'sup', 'known', 'list_start'):
        assert np.array_equal(got[k].numpy(), want[k]), k


def test_detection_table_argument_errors_do_not_launch():
    from opental_amd.csrc import build
    if not os.path.exists(build.LIB):
        build.build(verbose=False)
    from opental_amd._lib import declare
    lib = declare(ctypes.CDLL(build.LIB))
    f = lib.otal_detection_table
    one = ctypes.c_void_p(16)       # never dereferenced: argument checks come first

    def call(ptrs=None, V=3, K=5, top_k=7, cols=5, drop_empty=0, scoring=0):
        p = [one] * 9 if ptrs is None else ptrs        # rows, counts, durations, then the six outputs
        return f(p[0], p[1], p[2], V, K, top_k, cols, drop_empty, scoring, *p[3:], None)

    for k in (0, 1, 3, 4, 5, 6, 7, 8):                  # every pointer but durations, which may be NULL
        ptrs = [one] * 9
        ptrs[k] = None
        assert call(ptrs) == -1, k                      # OTAL_E_NULL
    for kw in (dict(V=0), dict(K=0), dict(top_k=0), dict(V=-1), dict(cols=2), dict(cols=6)):
        assert call(**kw) == -2, kw                     # OTAL_E_SHAPE
    for kw in (dict(scoring=-1), dict(scoring=6), dict(V=1 << 16, K=1 << 10, top_k=1 << 5)):
        assert call(**kw) == -7, kw                     # OTAL_E_UNSUPPORTED
