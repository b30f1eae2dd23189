"""GPU: otal_anchor_stats (csrc/anchorstats.hip) against anchor_stats_reference (opental_amd/common/anchor_stats.py) for every
anchor of every case -- labels and both histograms exactly, value and grad within the tolerances below, every output
pre-filled so that an unwritten or over-written element shows -- its accumulation, its run-to-run identity, its error codes,
and the analyze_anchors driver end to end on a random-weight network.

Tolerances.  value is the arithmetic of the decode kernel: rtol 1e-5, atol 1e-7 (tests/test_infer_gpu.py).  grad is a
difference of two numbers in (0, 1]: four times the reference's own float32-against-float64 spread (1.0e-7 of max |g|,
tests/golden/PIN_REPORT_anchor_stats.txt), no less than the 2e-5 of the ablation tests, times the case's largest |g|."""
import os

import numpy as np
import pytest
import torch

from anchor_stats_cases import BINS, CLIP, INPUTS, OVERLAP, SENTINEL, case, make_case, reference, targets_of

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VALUE_TOL = dict(rtol=1e-5, atol=1e-7)
ROWS = ('label', 'value', 'grad')


@pytest.fixture(scope="module")
def spread():
    return float(np.load(os.path.join(REPO, "tests", "golden", "anchor_stats.npz"))['spread_grad'])


def _pattern(shape, mod, add):
    """A known non-zero pattern: the histograms must come back as pattern + counts."""
    return (torch.arange(int(np.prod(shape)), dtype=torch.int64) % mod + add).reshape(shape)


def _sentinel_out(B, K, score_bins=BINS, grad_bins=BINS):
    return dict(hist_score=_pattern((2, 3, score_bins), 7, 1).cuda(), hist_grad=_pattern((2, grad_bins), 5, 3).cuda(),
                label=torch.full((B, K, 2), SENTINEL, dtype=torch.int32, device='cuda'),
                value=torch.full((B, K, 2), float(SENTINEL), device='cuda'),
                grad=torch.full((B, K, 2), float(SENTINEL), device='cuda'))


def _inputs(c):
    return [None if c[k] is None else torch.from_numpy(c[k]).cuda() for k in INPUTS]


def _launch(c, target, out=None, rows=True):
    from opental_amd.common import ops
    B, K = c['loc'].shape[:2]
    out = _sentinel_out(B, K) if out is None else out
    res = ops.anchor_stats(*_inputs(c), c['clip_length'], c['overlap_thresh'], c['os_head'], c['n_known'], target, BINS, BINS,
                           out=out, rows=rows)
    return {k: (None if v is None else v.cpu().numpy()) for k, v in res.items()}


def _check(c, target, spread):
    want = reference(c, target)
    got = _launch(c, target)
    B, K = c['loc'].shape[:2]
    assert np.array_equal(got['label'], want['label'])
    assert np.array_equal(got['hist_score'], _pattern((2, 3, BINS), 7, 1).numpy() + want['hist_score'])
    assert np.array_equal(got['hist_grad'], _pattern((2, BINS), 5, 3).numpy() + want['hist_grad'])
    assert int(want['hist_score'].sum()) == 2 * B * K and int(want['hist_grad'].sum()) == int(want['counts'].sum())
    gmax = max(float(np.abs(want['grad']).max()), 1e-30)
    print(f"{target}: max |value diff| {float(np.abs(got['value'] - want['value']).max()):.3e}, "
          f"max |grad diff| / max |g| {float(np.abs(got['grad'] - want['grad']).max()) / gmax:.3e}")
    np.testing.assert_allclose(got['value'], want['value'], **VALUE_TOL)
    assert np.abs(got['grad'] - want['grad']).max() <= max(2e-5, 4.0 * spread) * gmax
    assert (got['grad'][~want['counts']] == 0.0).all()              # rows that do not count hold 0, not the sentinel
    return got, want


def test_smallest_launch(spread):
    c = case('smallest')
    for target in targets_of(c):
        _check(c, target, spread)


@pytest.mark.parametrize("target", ['uncertainty', 'actionness', 'confidence', 'uncertainty_actionness', 'half_au'])
@pytest.mark.parametrize("name", ['thumos_no_positive', 'thumos_no_gt'])
def test_thumos_launch_every_target(name, target, spread):
    """(2, 126, 15, 4); sample 1 has no positive anchor, or gvalid all zero over segments that would match."""
    c = case(name)
    got, want = _check(c, target, spread)
    assert not got['label'][1].any() and got['label'][0].any()
    assert (want['hist_score'].sum(-1) > 0).all()                   # known, unknown and background in both stages


@pytest.mark.parametrize("name,target", [('k257', 'half_au'), ('k516', 'confidence'), ('c33', 'confidence'),
                                         ('c33', 'uncertainty'), ('g40', 'uncertainty_actionness'), ('g40', 'actionness')])
def test_shapes_past_one_pass(name, target, spread):
    """K = 257 and 516: more than one pass of the 256-thread workgroup, no multiple of the wavefront; C = 33: more classes
    than half a wavefront; G = 40: more ground truths than any per-lane assumption."""
    got, want = _check(case(name), target, spread)
    assert (want['label'] > 0).any() and want['counts'].any()


@pytest.mark.parametrize("target", ['uncertainty', 'confidence'])
def test_closed_head_every_anchor_has_a_gradient_row(target, spread):
    """os_head false, C = 16 with class 0 as background: column = the label itself, background anchors included."""
    c = case('closed')
    got, want = _check(c, target, spread)
    assert want['counts'][want['label'] == 0].all() and (got['grad'][want['label'] == 0] != 0.0).all()


def test_unknown_group_inside_the_head(spread):
    """n_known = 8 below the largest label: unknown anchors that still have a gradient row (labels 9..15)."""
    got, want = _check(case('few_known'), 'uncertainty', spread)
    assert (want['counts'] & (want['group'] == 1)).any() and want['hist_score'][:, 1].sum() >= 10


def test_tied_areas_take_the_first(spread):
    got, want = _check(case('tie'), 'uncertainty', spread)
    tied = (want['area_gap'][0] == 0) & (want['label'][0, :, 0] > 0)
    assert tied.sum() >= 3 and (got['label'][0, tied, 0] == 1).all()


def _clamp_edit(c):
    for k in ('conf', 'prop_conf'):
        c[k][:, 0::5, 0] = 30.0
        c[k][:, 1::5, 1] = -30.0
        c[k][:, 2::5, 1:] = -30.0
        c[k][:, 2::5, 0] = 0.0


@pytest.mark.parametrize("target", ['uncertainty', 'confidence', 'half_au'])
def test_logits_past_the_clamp(target, spread):
    """+-30 logits: the evidence is exp(+-10).  Every fifth anchor has one logit of 30 (unclamped, 15 / S would be ~1e-12), every
    fifth a 0 and fourteen logits of -30 (unclamped, their alpha would be exactly 1.0f instead of 1 + e^-10): the uncertainty the
    kernel returns is far, in units of the tolerance, from the unclamped one."""
    c = make_case(2, 126, 15, 4, seed=0, edit=_clamp_edit)
    got, want = _check(c, target, spread)
    u = _launch(c, 'uncertainty')['value'].astype(np.float64)
    for s, k in enumerate(('conf', 'prop_conf')):
        unclamped = 15.0 / (np.exp(c[k].astype(np.float64)) + 1.0).sum(-1)
        rel = np.abs(u[:, :, s] - unclamped) / unclamped
        assert (rel[:, 0::5] > 0.5).all() and (rel[:, 2::5] > 2e-5).all() and (rel[:, 3::5] < 1e-5).all()
    assert (u[:, 0::5] > 1e-5).all() and (u[:, 0::5] < 1e-3).all()


def _saturate_edit(c):
    for k, shift in (('act', 0), ('prop_act', 1)):
        c[k][:, (0 + shift)::4] = 30.0
        c[k][:, (1 + shift)::4] = -30.0
        c[k][:, (2 + shift)::4] = -100.0


@pytest.mark.parametrize("target", ['actionness', 'uncertainty_actionness', 'half_au', 'confidence'])
def test_saturated_actionness_hits_both_end_bins(target, spread):
    """An actionness logit of +30 gives exactly 1.0f: bin 100 is clamped into the last bin.  -30 gives 9.4e-14 in float32 (not
    0.0f: 1 / (1 + e^30) is representable) and -100 gives exactly 0.0f (e^100 overflows to inf): both in bin 0."""
    c = make_case(2, 126, 15, 4, seed=0, edit=_saturate_edit, ends_exempt=True)
    got, want = _check(c, target, spread)
    a = _launch(c, 'actionness')
    assert (a['value'][:, 0::4, 0] == 1.0).all() and (a['value'][:, 1::4, 1] == 1.0).all()
    assert (a['value'][:, 2::4, 0] == 0.0).all() and (a['value'][:, 1::4, 0] > 0.0).all() and (a['value'][:, 1::4, 0] < 1e-12).all()
    hist = a['hist_score'] - _pattern((2, 3, BINS), 7, 1).numpy()
    assert hist[0, :, BINS - 1].sum() >= 2 * 32 and hist[0, :, 0].sum() >= 2 * 2 * 31


def test_two_launches_accumulate():
    c = case('k257')
    want = reference(c, 'half_au')
    B, K = c['loc'].shape[:2]
    out = _sentinel_out(B, K)
    _launch(c, 'half_au', out=out)
    twice = _launch(c, 'half_au', out=out)
    zero = lambda: dict(hist_score=torch.zeros((2, 3, BINS), dtype=torch.int64, device='cuda'),
                        hist_grad=torch.zeros((2, BINS), dtype=torch.int64, device='cuda'))
    one, two = _launch(c, 'half_au', out=zero()), _launch(c, 'half_au', out=zero())
    assert np.array_equal(one['hist_score'], want['hist_score']) and np.array_equal(one['hist_grad'], want['hist_grad'])
    assert np.array_equal(twice['hist_score'], _pattern((2, 3, BINS), 7, 1).numpy() + one['hist_score'] + two['hist_score'])
    assert np.array_equal(twice['hist_grad'], _pattern((2, BINS), 5, 3).numpy() + one['hist_grad'] + two['hist_grad'])


def test_two_runs_give_identical_bytes():
    c = case('k516')
    a, b = _launch(c, 'confidence'), _launch(c, 'confidence')
    for k in ROWS + ('hist_score', 'hist_grad'):
        assert a[k].tobytes() == b[k].tobytes(), k


def test_histograms_only():
    """The row arrays are nullable: the driver that only wants histograms passes none."""
    c = case('thumos_no_positive')
    full = _launch(c, 'uncertainty')
    B, K = c['loc'].shape[:2]
    out = {k: v for k, v in _sentinel_out(B, K).items() if k.startswith('hist')}
    got = _launch(c, 'uncertainty', out=out, rows=False)
    assert all(got[k] is None for k in ROWS)
    assert np.array_equal(got['hist_score'], full['hist_score']) and np.array_equal(got['hist_grad'], full['hist_grad'])


def test_error_codes_leave_the_outputs_alone():
    from opental_amd import _lib as L
    c = case('thumos_no_positive')
    B, K, C = c['conf'].shape
    G = c['gt'].shape[1]
    ins = _inputs(c)
    out = _sentinel_out(B, K)
    before = {k: v.clone() for k, v in out.items()}
    outs = [out[k] for k in ('hist_score', 'hist_grad', 'label', 'value', 'grad')]

    def call(ins=ins, dims=(B, K, C, G), os_head=1, n_known=15, target=0, bins=(BINS, BINS), outs=outs):
        p = lambda t: None if t is None else L.ptr(t)
        return L.lib().otal_anchor_stats(*[p(t) for t in ins], *dims, CLIP, OVERLAP, os_head, n_known, target, *bins,
                                         *[p(t) for t in outs], L.stream())
    null, shape, unsupported = -1, -2, L.E_UNSUPPORTED
    for i in (0, 1, 2, 3, 6, 7, 8):                                 # every required input; act / prop_act are not
        assert call(ins=[None if j == i else t for j, t in enumerate(ins)]) == null, i
    for i in (0, 1):
        assert call(outs=[None if j == i else t for j, t in enumerate(outs)]) == null, i
    for i in range(4):
        for bad in (0, -1):
            assert call(dims=tuple(bad if j == i else d for j, d in enumerate((B, K, C, G)))) == shape, i
    assert call(bins=(0, BINS)) == shape and call(bins=(BINS, 0)) == shape
    assert call(target=5) == unsupported and call(target=-1) == unsupported
    assert call(n_known=0) == unsupported
    no_act = [None if j in (4, 5) else t for j, t in enumerate(ins)]
    for target in (1, 3, 4):
        assert call(ins=no_act, os_head=0, target=target) == unsupported, target
    assert call(ins=no_act, os_head=1, target=2) == unsupported     # confidence with os_head multiplies by the actionness
    assert call(ins=[None if j == 5 else t for j, t in enumerate(ins)]) == unsupported      # one map without the other
    assert call(bins=(4096, 1)) == unsupported                      # 6 * 4096 + 2 counters do not fit the workgroup's LDS
    torch.cuda.synchronize()
    for k, v in out.items():
        assert torch.equal(v, before[k]), k
    assert call(ins=no_act, os_head=0, target=0) == 0               # and the maps are optional where nothing reads them
    assert call() == 0


CLASSES_ALL = [(7 + 2 * i, f"Class{i:02d}") for i in range(20)]     # the first 15 are the split's known classes


def _write_dataset(root):
    """Two short videos (300 and 256 sampled frames, count = sample_count) and a hand-written annotation file: 'v_a' has
    windows at 0 and 44; window 0 holds its first two actions whole, window 44 the last two whole and 75 % of the first.
    Classes 16 and 18 of the full list are held out."""
    import yaml
    rs = np.random.RandomState(11)
    os.makedirs(root / 'npy')
    os.makedirs(root / 'split_0')
    for name, frames in (('v_a', 300), ('v_b', 256)):
        np.save(root / 'npy' / (name + '.npy'), rs.randint(0, 256, (frames, 96, 96, 3)).astype(np.uint8))
    (root / 'split_0' / 'Class_Index_Known.txt').write_text("".join(f"{i} {n}\n" for i, n in CLASSES_ALL[:15]))
    (root / 'split_0' / 'Class_Index_All.txt').write_text("".join(f"{i} {n}\n" for i, n in CLASSES_ALL))
    (root / 'info.csv').write_text("video,fps,sample_fps,count,sample_count\nv_a,10.0,10.0,300,300\nv_b,10.0,10.0,256,256\n")
    rows = [('v_a', 2, 30, 90), ('v_a', 15, 120, 200), ('v_a', 9, 250, 290), ('v_b', 0, 10, 100), ('v_b', 17, 150, 250)]
    (root / 'anno_open.csv').write_text("video,type,type_idx,start,end,startFrame,endFrame\n" + "".join(
        f"{v},{CLASSES_ALL[c][1]},{CLASSES_ALL[c][0]},{s / 10:.1f},{e / 10:.1f},{s},{e}\n" for v, c, s, e in rows))
    with open(os.path.join(REPO, 'configs', 'thumos14_opental_final.yaml')) as f:
        cfg = yaml.load(f.read(), Loader=yaml.FullLoader)
    cfg['dataset']['class_info_path'] = str(root / 'split_{id:d}' / 'Class_Index_Known.txt')
    cfg['dataset']['testing'].update(video_info_path=str(root / 'info.csv'), video_anno_path=str(root / 'anno_open.csv'),
                                     video_anno_open_path=str(root / 'anno_open.csv'), video_data_path=str(root / 'npy'))
    (root / 'anchors.yaml').write_text(yaml.dump(cfg))
    return str(root / 'anchors.yaml')


def test_analyze_anchors_end_to_end(tmp_path, monkeypatch, spread):
    """python -m opental_amd.thumos14.analyze_anchors on a random-weight THUMOS14 BDNet (the coarse boundary head gets a
    positive bias, so that the refined stage keeps some labels).  The network runs once; its head outputs are recorded on the
    way, and the host rule over them is the yardstick for the driver's .npz."""
    from opental_amd.common import ops
    from opental_amd.common.anchor_stats import anchor_stats_reference, grad_edges, score_edges
    from opental_amd.thumos14 import analyze_anchors as AN
    precision = ops.CONV_PRECISION
    yaml_path = _write_dataset(tmp_path)
    seen, calls = [], []
    forward_windows, load_net = AN.forward_windows, AN.load_net

    def recording(*args, **kwargs):
        heads = forward_windows(*args, **kwargs)
        seen.append({k: v.clone() for k, v in heads.items()})
        return heads

    def counting(*args, **kwargs):
        net = load_net(*args, **kwargs)
        with torch.no_grad():           # extents of e^2 strides instead of one: some anchors pass the IoU test, some do not
            net.coarse_pyramid_detection.loc_head.conv1d.bias.fill_(2.0)
        net.register_forward_hook(lambda *a: calls.append(1))
        return net
    monkeypatch.setattr(AN, 'forward_windows', recording)
    monkeypatch.setattr(AN, 'load_net', counting)
    torch.manual_seed(0)
    npz = tmp_path / 'out' / 'anchors.npz'
    try:
        path, _ = AN.main([yaml_path, '--open_set', '--split', '0', '--piou', '0.5', '--random_init', '--subset', 'test',
                           '--target', 'half_au', '--keep_rows', '--output_npz', str(npz), '--plots', str(tmp_path / 'plots')])
    finally:
        ops.CONV_PRECISION = precision
    assert len(seen) == 1 and len(calls) == 1                       # one batch of windows, one pass through the network
    heads = {k: v.float().cpu().numpy() for k, v in seen[0].items()}
    windows = [('v_a', 0, [[30, 90, 3], [120, 200, 16]]), ('v_a', 44, [[1, 46, 3], [76, 156, 16], [206, 246, 10]]),
               ('v_b', 0, [[10, 100, 1], [150, 250, 18]])]
    gt = np.zeros((3, 3, 3), np.float32)
    gvalid = np.zeros((3, 3), np.uint8)
    for b, (_, _, annos) in enumerate(windows):
        for g, (s, e, lab) in enumerate(annos):
            gt[b, g] = (s / 256.0, e / 256.0, lab)
            gvalid[b, g] = 1
    assert heads['conf'].shape == (3, 126, 15)
    want = anchor_stats_reference(heads['loc'], heads['conf'], heads['prop_conf'], heads['center'], heads['act'],
                                  heads['prop_act'], heads['priors'], gt, gvalid, 256, 0.5, True, 15, 'half_au')
    data = np.load(path)
    assert data['window_video'].tolist() == [w[0] for w in windows] and data['window_offset'].tolist() == [w[1] for w in windows]
    assert np.array_equal(data['label'], want['label'])
    assert np.array_equal(data['hist_score'], want['hist_score']) and np.array_equal(data['hist_grad'], want['hist_grad'])
    assert np.array_equal(data['group_counts'], want['hist_score'].sum(-1)) and int(data['group_counts'].sum()) == 2 * 3 * 126
    assert (want['label'] > 15).any() and ((want['label'] > 0) & (want['label'] <= 15)).any()
    assert (want['label'][:, :, 1] > 0).any() and (want['label'][:, :, 0] != want['label'][:, :, 1]).any()
    np.testing.assert_allclose(data['value'], want['value'], **VALUE_TOL)
    gmax = max(float(np.abs(want['grad']).max()), 1e-30)
    assert np.abs(data['grad'] - want['grad']).max() <= max(2e-5, 4.0 * spread) * gmax
    assert np.array_equal(data['score_edges'], score_edges(100)) and np.array_equal(data['grad_edges'], grad_edges(100).astype(np.float64))
    assert (str(data['target']), float(data['piou']), int(data['score_bins']), int(data['grad_bins']), int(data['split']),
            str(data['subset']), int(data['n_windows'])) == ('half_au', 0.5, 100, 100, 0, 'test', 3)
    for name in ('dist_coarse.png', 'dist_refined.png', 'grad_density.png', 'grad_prop_density.png'):
        assert os.path.getsize(tmp_path / 'plots' / name) > 0
