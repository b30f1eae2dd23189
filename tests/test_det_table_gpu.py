"""GPU: otal_detection_table (csrc/dettable.hip) against table_reference (opental_amd/common/det_table.py), element by
element -- every output column, list_start and N, with the outputs pre-filled so that a write past N shows -- its
run-to-run identity, and the ActivityNet thresholding pass end to end on a random-weight network."""
import json

import numpy as np
import pytest
import torch

from det_table_cases import SCORINGS, SENTINEL, make_case

pytestmark = pytest.mark.gpu

COLUMNS = ('video', 'cls', 'seg', 'sup', 'known')


def _sentinel_out(V, K, top_k):
    cap = V * K * top_k
    mk = lambda shape, dtype: torch.full(shape, SENTINEL, dtype=dtype, device='cuda')
    return dict(video=mk((cap,), torch.int32), cls=mk((cap,), torch.int32), seg=mk((cap, 2), torch.float64),
                sup=mk((cap, 3), torch.float32), known=mk((cap,), torch.float64), list_start=mk((V * K + 1,), torch.int32))


def _device_table(rows, counts, durations, drop_empty, scoring):
    from opental_amd.common import ops
    V, K, top_k, _ = rows.shape
    table = ops.detection_table(torch.from_numpy(rows).cuda(), torch.from_numpy(counts).cuda(),
                                None if durations is None else durations.tolist(), drop_empty, scoring,
                                out=_sentinel_out(V, K, top_k))
    assert table['n'].is_cuda and table['n'].dim() == 0
    return {k: v.cpu().numpy() for k, v in table.items()}


def _check(rows, counts, durations=None, drop_empty=False, scoring='uncertainty'):
    from opental_amd.common.det_table import table_reference
    want = table_reference(rows, counts, durations, drop_empty, scoring)
    got = _device_table(rows, counts, durations, drop_empty, scoring)
    n = int(got['n'])
    assert n == want['n']
    assert np.array_equal(got['list_start'], want['list_start'])
    for k in COLUMNS:
        assert got[k].dtype == want[k].dtype, k
        assert np.array_equal(got[k][:n], want[k]), k
        assert (got[k][n:] == SENTINEL).all(), k         # rows at and past N were not written
    return got, want


@pytest.mark.parametrize("count", [0, 1])
def test_one_row(count):
    rows, counts, durations = make_case(1, 1, 1, 5, seed=1, counts=count)
    got, _ = _check(rows, counts, durations)
    assert int(got['n']) == count


@pytest.mark.parametrize("variant", ["plain", "durations", "drop_empty"])
@pytest.mark.parametrize("cols", [3, 4, 5])
def test_small_lists(cols, variant):
    rows, counts, durations = make_case(3, 5, 7, cols, seed=cols)
    got, _ = _check(rows, counts, durations if variant == "durations" else None, variant == "drop_empty")
    assert int(got['n']) >= 0.4 * 3 * 5 * 7


@pytest.mark.parametrize("scoring", SCORINGS)
def test_every_scoring(scoring):
    from opental_amd.common.det_table import threshold_from_scores
    rows, counts, durations = make_case(3, 5, 7, 5, seed=5)
    got, want = _check(rows, counts, durations, scoring=scoring)
    n = int(got['n'])
    assert len(set(want['known'].tolist())) > n // 2                 # the column is not a constant
    assert threshold_from_scores(torch.from_numpy(got['known'][:n]).cuda()) == threshold_from_scores(want['known'])


@pytest.mark.parametrize("shape", [(2, 2, 257), (2, 2, 516), (2, 150, 189)])
@pytest.mark.parametrize("cols", [3, 5])
def test_lists_longer_than_a_workgroup_pass(shape, cols):
    """257 and 516 rows: more than one pass of 256 threads, no multiple of the wavefront; (2, 150, 189) is the ActivityNet
    list shape."""
    rows, counts, durations = make_case(*shape, cols, seed=shape[2])
    got, _ = _check(rows, counts, durations, scoring='half_au')
    assert int(got['n']) >= 0.4 * shape[0] * shape[1] * shape[2]


def test_no_detections():
    from opental_amd.common.det_table import threshold_from_scores
    rows, counts, durations = make_case(2, 3, 9, 5, seed=2, counts=0)
    got, _ = _check(rows, counts, durations)
    assert int(got['n']) == 0 and not got['list_start'].any()
    with pytest.raises(ValueError, match="no detections to threshold"):
        threshold_from_scores(torch.from_numpy(got['known'][:0]).cuda())


def test_two_calls_give_identical_tables():
    rows, counts, durations = make_case(2, 150, 189, 5, seed=9)
    a = _device_table(rows, counts, durations, False, 'u_by_inv_a')
    b = _device_table(rows, counts, durations, False, 'u_by_inv_a')
    assert int(a['n']) > 0
    for k in COLUMNS + ('list_start',):
        assert np.array_equal(a[k], b[k]), k


def test_thresholding_pass_end_to_end(tmp_path, monkeypatch):
    """opental_amd.anet.threshold.thresholding on a random-weight ActivityNet BDNet and two synthetic videos (500 and exactly
    768 frames).  Both actionness heads get a positive bias, so that detections exist by construction.  The network runs
    once; its Soft-NMS rows are recorded on the way, and the host loops over those rows are the yardstick."""
    from opental_amd.anet import test as A
    from opental_amd.anet import threshold as TH
    from opental_amd.anet.BDNet import BDNet
    from opental_amd.thumos14.test import ood_threshold
    rs = np.random.RandomState(3)
    npy = tmp_path / 'npy'
    npy.mkdir()
    infos = {}
    for name, frames in (('v_short', 500), ('v_full', 768)):
        np.save(npy / (name + '.npy'), rs.randint(0, 256, (frames, 96, 96, 3)).astype(np.uint8))
        infos[name] = {'subset': 'training', 'duration': frames / 10.0, 'fps': 10.0}
    (tmp_path / 'info.json').write_text(json.dumps(infos))
    names, infos = TH.select_videos(str(tmp_path / 'info.json'), str(npy))
    assert names == ['v_short', 'v_full']
    torch.manual_seed(0)
    net = BDNet(training=False, use_edl=True)
    with torch.no_grad():
        net.coarse_pyramid_detection.actionness_head.conv1d.bias.fill_(2.0)
        net.coarse_pyramid_detection.prop_actionness_head.conv1d.bias.fill_(2.0)
    net = net.cuda().eval()
    seen = []
    detect_rows = A.detect_rows

    def recording(*args, **kwargs):
        rows, counts = detect_rows(*args, **kwargs)
        seen.append((rows.clone(), counts.clone()))
        return rows, counts
    monkeypatch.setattr(A, 'detect_rows', recording)
    out = tmp_path / 'out' / 'threshold.json'
    thr = TH.thresholding(net, names, infos, str(npy), str(out), scoring='uncertainty_actionness', keep_detections=True)
    assert len(seen) == 1                                             # one batch, one pass through the network
    rows, counts = seen[0]
    assert tuple(rows.shape) == (2, 150, 189, 5)
    dicts = {n[2:]: A.get_video_prediction(rows[v], counts[v], infos[n]['duration']) for v, n in enumerate(names)}
    assert sum(len(p) for p in dicts.values()) >= 100
    assert thr == ood_threshold(dicts, 'uncertainty_actionness')
    data = json.loads(out.read_text())
    assert data['version'] == 'ActivityNet-v1.3' and data['external_data'] == {'threshold': thr}
    assert data['results'] == dicts
    assert TH.read_threshold_file(str(out)) == thr
