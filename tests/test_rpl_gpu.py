"""GPU: the RPL and GCPL baselines -- the distance-head kernels (csrc/rplhead.hip) against the float64 restatement
tests/rpl_ref.py, the fused loss otal_detection_loss_rpl against tests/golden/rpl.npz (tools/pin_rpl.py) and the package's own
torch formulation, the model forward, the captured training step and the train / test / threshold drivers."""
import json
import os
import re
import sys

import numpy as np
import pytest
import torch
import yaml

import rpl_ref as R
from oracle import arch
from test_rpl_cpu import VARIANTS, check_grads, head_outputs, package_loss, priors, targets_of

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C = R.C
W = dict(lw=1.0, cw=10.0, ctw=1.0, actw=1.0, ssl=0.001)


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "rpl.npz"))


@pytest.fixture(scope="module")
def ref_err(golden_dir, fx):
    """The reference's own fp32 error against float64 (dist, dx, dcenters) as written in PIN_REPORT_rpl.txt."""
    txt = open(os.path.join(golden_dir, "PIN_REPORT_rpl.txt")).read()
    m = re.search(r"max \|dist err\| (\S+), max \|dx err\| (\S+), max \|dcenters err\| (\S+) ", txt)
    errs = [float(v.rstrip(",")) for v in m.groups()]
    np.testing.assert_allclose(errs, fx["head_ref_fp32_err"], rtol=1e-6)
    return errs


def _head(x, cen):
    from opental_amd.common import ops
    return ops.RPLHeadFunction.apply(x, cen)


def _graph_has(fn, name, depth=6):
    if fn is None or depth < 0:
        return False
    return name in type(fn).__name__ or any(_graph_has(n, name, depth - 1) for n, _ in fn.next_functions)


def test_head_forward_against_float64(fx, ref_err):
    """Bound: 4 x the reference's fp32 error of its expanded form (the two fp32 summation orders differ by a few ulps)."""
    dev = torch.device("cuda", 0)
    fc, _, cc, _, _ = R.seeded_inputs()
    d = _head(torch.from_numpy(fc).to(dev), torch.from_numpy(cc).to(dev))
    assert d.shape == (R.B, C, R.N) and float(d.min()) >= 0.0
    want = R.head_fwd(fc, cc)
    np.testing.assert_allclose(want, fx["head_dist_f64"], rtol=0, atol=1e-13)
    err = float(np.abs(d.cpu().numpy().astype(np.float64) - want).max())
    print(f"rpl head forward: max |err| vs float64 {err:.3e} (reference fp32 {ref_err[0]:.3e})")
    assert err <= 4 * ref_err[0], f"head forward max |err| {err:.3e} > 4 x {ref_err[0]:.3e}"


def test_head_backward_against_float64(ref_err):
    dev = torch.device("cuda", 0)
    fc, _, cc, _, g = R.seeded_inputs()
    x = torch.from_numpy(fc).to(dev).requires_grad_(True)
    cen = torch.from_numpy(cc).to(dev).requires_grad_(True)
    _head(x, cen).backward(torch.from_numpy(g).to(dev))
    dx, dcen = R.head_bwd(fc, cc, g)
    e_dx = float(np.abs(x.grad.cpu().numpy().astype(np.float64) - dx).max())
    e_dc = float(np.abs(cen.grad.cpu().numpy().astype(np.float64) - dcen).max())
    print(f"rpl head backward: max |err| vs float64 dx {e_dx:.3e} (reference fp32 {ref_err[1]:.3e}), "
          f"dcenters {e_dc:.3e} (reference fp32 {ref_err[2]:.3e})")
    assert e_dx <= 4 * ref_err[1], f"dx max |err| {e_dx:.3e} > 4 x {ref_err[1]:.3e}"
    assert e_dc <= 4 * ref_err[2], f"dcenters max |err| {e_dc:.3e} > 4 x {ref_err[2]:.3e}"


@pytest.mark.parametrize("shape", [(2, 16, 512, 126), (8, 16, 512, 126), (3, 21, 48, 70), (1, 5, 512, 33)])
def test_head_is_deterministic_and_handles_ragged_shapes(shape):
    """Two runs give the same bits; shapes whose N is no multiple of the 32-column tile and whose C, D are not the model's
    agree with float64 (the bound of an fp32 sum of D squared differences: D ulps of the result is generous)."""
    dev = torch.device("cuda", 0)
    Bn, Cn, Dn, Nn = shape
    rs = np.random.RandomState(Bn * 1000 + Nn)
    xn = np.maximum(rs.standard_normal((Bn, Dn, Nn)), 0).astype(np.float32)
    cn = (0.1 * rs.standard_normal((Cn, Dn))).astype(np.float32)
    gn = rs.standard_normal((Bn, Cn, Nn)).astype(np.float32)
    runs = []
    for _ in range(2):
        x = torch.from_numpy(xn).to(dev).requires_grad_(True)
        cen = torch.from_numpy(cn).to(dev).requires_grad_(True)
        d = _head(x, cen)
        d.backward(torch.from_numpy(gn).to(dev))
        runs.append((d.detach().clone(), x.grad.clone(), cen.grad.clone()))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    want = (R.head_fwd(xn, cn),) + R.head_bwd(xn, cn, gn)
    for got, ref in zip(runs[0], want):
        tol = Dn * np.finfo(np.float32).eps * max(float(np.abs(ref).max()), 1e-6)
        assert float(np.abs(got.cpu().numpy().astype(np.float64) - ref).max()) <= tol


@pytest.mark.parametrize("name", ["rpl", "gcpl"])
def test_fused_loss_matches_golden(fx, name):
    """Terms and TOTAL gradients (through RPLHeadFunction into features and centres), test_closed_set_gpu's tolerances."""
    dev = torch.device("cuda", 0)
    terms, ins, out = package_loss(name, targets_of(fx), dev=dev)
    assert 'RPLDetectionLossFunction' in type(terms[0].grad_fn).__name__
    assert _graph_has(out["conf"].grad_fn, 'RPLHeadFunction') and _graph_has(out["prop_conf"].grad_fn, 'RPLHeadFunction')
    assert terms[5] is None and terms[6] is None
    got = [float(t.detach()) for t in terms[:5]]
    assert np.allclose(got, fx[f"loss_{name}_terms"], rtol=2e-5, atol=1e-6), (got, fx[f"loss_{name}_terms"])
    sum(float(w) * t for w, t in zip(fx["weights"], terms[:5])).backward()
    check_grads(fx, name, ins, rtol=2e-5)


@pytest.mark.parametrize("name", ["rpl", "gcpl"])
@pytest.mark.parametrize("B", [1, 2, 8])
def test_fused_loss_matches_torch_formulation(name, B):
    from opental_amd.common.layers import RPLHead
    from opental_amd.thumos14 import multisegment_loss as M
    dev = torch.device("cuda", 0)
    rs = np.random.RandomState(B)
    heads = head_outputs(B, seed=100 + B)
    targets = []
    for b in range(B):
        if b == B - 1 and B > 1:
            rows = [[0.2505, 0.2575, 3.0]]      # no anchor centre inside: this sample has no positive
        else:
            rows = []
            for _ in range(1 + b % 3):
                st = rs.uniform(0.0, 0.8)
                rows.append([st, st + rs.uniform(0.05, 0.2), float(rs.randint(1, C))])
        targets.append(torch.tensor(rows, dtype=torch.float32, device=dev))
    feats = [np.maximum(rs.standard_normal((B, R.D, R.N)), 0).astype(np.float32) for _ in range(2)]
    cens = [(0.1 * rs.standard_normal((C, R.D))).astype(np.float32) for _ in range(2)]

    def run(fused):
        M.FUSED = fused
        try:
            ins = {k: torch.from_numpy(heads[k].copy()).to(dev).requires_grad_(True) for k in ("loc", "prop_loc", "center")}
            ins["feat"] = torch.from_numpy(feats[0]).to(dev).requires_grad_(True)
            ins["prop_feat"] = torch.from_numpy(feats[1]).to(dev).requires_grad_(True)
            hc, hp = RPLHead(R.D, C).to(dev), RPLHead(R.D, C).to(dev)
            hc.centers.data.copy_(torch.from_numpy(cens[0]))
            hp.centers.data.copy_(torch.from_numpy(cens[1]))
            ins["centers"], ins["prop_centers"] = hc.centers, hp.centers
            tr = lambda y: y.permute(0, 2, 1).contiguous()
            out = dict(loc=ins["loc"], prop_loc=ins["prop_loc"], center=ins["center"], priors=priors().to(dev), act=None,
                       prop_act=None, conf=tr(hc(ins["feat"])), prop_conf=tr(hp(ins["prop_feat"])))
            crit = M.MultiSegmentLoss(C, 0.5, 1.0, cls_loss_type='rpl', rpl_config=dict(VARIANTS[name])).to(dev)
            terms = crit(out, targets)
            assert ('RPLDetectionLossFunction' in type(terms[0].grad_fn).__name__) == fused
            sum(l * w for l, w in zip(terms[:5], (1.0, 10.0, 1.0, 10.0, 1.0))).backward()
            return [float(t.detach()) for t in terms[:5]], {k: v.grad.clone() for k, v in ins.items()}
        finally:
            M.FUSED = True
    l0, g0 = run(False)
    l1, g1 = run(True)
    assert np.allclose(l0, l1, rtol=2e-5, atol=1e-6), (l0, l1)
    for k in g0:
        scale = float(g0[k].abs().max())
        assert scale > 0, k
        assert float((g0[k] - g1[k]).abs().max()) <= 2e-5 * scale, (k, scale)


def rpl_params(seed=2020):
    """tools/pin_rpl.py rpl_params: arch.make_params without the actionness and conf-head convolutions + the seeded centres."""
    p = {k: v for k, v in arch.make_params(seed).items()
         if "actionness_head" not in k and ".conf_head." not in k and ".prop_conf_head." not in k}
    _, _, cc, cp, _ = R.seeded_inputs()
    p["coarse_pyramid_detection.conf_head.centers"] = cc
    p["coarse_pyramid_detection.prop_conf_head.centers"] = cp
    return p


def rpl_net(in_channels=3, seed=0, training=False):
    from opental_amd.thumos14.BDNet import BDNet, DEFAULT_MODEL_CFG
    torch.manual_seed(seed)
    net = BDNet(in_channels=in_channels, training=False, use_rpl=True, cfg=dict(DEFAULT_MODEL_CFG, os_head=False))
    net.backbone._model.apply(BDNet.weight_init)
    return net


def test_model_forward_matches_golden(fx):
    from opental_amd.common import ops
    from opental_amd.thumos14.BDNet import BDNet, DEFAULT_MODEL_CFG
    dev = torch.device("cuda", 0)
    old = ops.CONV_PRECISION
    ops.CONV_PRECISION = 0
    try:
        net = BDNet(training=False, use_rpl=True, cfg=dict(DEFAULT_MODEL_CFG, os_head=False))
        net.load_state_dict({k: torch.from_numpy(v) for k, v in rpl_params().items()})
        net = net.to(dev).eval()
        x = torch.from_numpy(arch.make_clip(int(fx["model_clip_seed"]), 1)).to(dev)
        with torch.no_grad():
            out = net(x)
        assert out['act'] is None and out['prop_act'] is None and 'cls_ctr' not in out
        for k in ("conf", "prop_conf"):
            assert out[k].shape == (1, 126, C) and float(out[k].min()) >= 0.0
        rel = lambda a, b: float(np.abs(np.asarray(a, np.float64) - b).max() / max(np.abs(b).max(), 1e-6))
        for k in ("loc", "conf", "prop_loc", "prop_conf", "center"):
            assert rel(out[k].cpu().numpy(), fx[f"model_out_{k}"]) < 1e-4, k
    finally:
        ops.CONV_PRECISION = old


def test_training_output_dict_carries_the_centres():
    from opental_amd.common import ops
    dev = torch.device("cuda", 0)
    old = ops.CONV_PRECISION
    ops.CONV_PRECISION = 0
    try:
        net = rpl_net().to(dev).train()
        out = net(torch.from_numpy(arch.make_clip(11, 1)).to(dev))
        cpd = net.coarse_pyramid_detection
        assert out['cls_ctr'] is cpd.conf_head.centers and out['prop_cls_ctr'] is cpd.prop_conf_head.centers
        assert out['ctr_feat'].shape == (1, 126, 512) and out['prop_ctr_feat'].shape == (1, 126, 512)
        # conf is the distance of ctr_feat to the centres
        want = ((out['ctr_feat'].detach()[:, :, None, :] - cpd.conf_head.centers.detach()[None, None]) ** 2).mean(-1)
        assert float((out['conf'].detach() - want).abs().max()) <= 1e-5 * float(want.abs().max())
    finally:
        ops.CONV_PRECISION = old


@pytest.mark.parametrize("name", ["rpl", "gcpl"])
def test_rpl_lane_graph_steps_equal_eager_steps(name):
    """The shape of test_closed_set_lane_graph_steps_equal_eager_steps: the capture's warm-up step plus three replayed
    lane-graph steps leave parameters and Adam moments BIT-IDENTICAL to four eager steps -- and the centres, ordinary
    parameters of the flat Adam arena, have moved."""
    import bench
    from opental_amd.common import ops
    from opental_amd.thumos14 import multisegment_loss as M
    from opental_amd.thumos14.train import DetectorTrainer
    dev = torch.device("cuda", 0)
    old = ops.CONV_PRECISION
    ops.CONV_PRECISION = 1
    try:
        clips, targets, scores = bench.synth_batch(2, 1000, dev)

        def run(lanes):
            net = rpl_net(seed=5).to(dev).train()
            cpd = net.coarse_pyramid_detection
            init = [cpd.conf_head.centers.detach().clone(), cpd.prop_conf_head.centers.detach().clone()]
            crit = M.MultiSegmentLoss(C, 0.5, 1.0, cls_loss_type='rpl', rpl_config=dict(VARIANTS[name])).to(dev)
            tr = DetectorTrainer(net, crit, W, lr=1e-4, weight_decay=1e-3)
            done = 0
            if lanes:
                tr.capture_step(clips, targets, scores, warmup=1, lanes=True)       # the warm-up step is a real step
                assert tr._graph[0] == "lanes"
                done = 1
            costs = [float(tr.step(clips, targets, scores)[0]) for _ in range(4 - done)]
            torch.cuda.synchronize()
            assert tr.step_count == 4
            flat = tr.arena.flat
            for p, p0 in zip((cpd.conf_head.centers, cpd.prop_conf_head.centers), init):
                off = (p.data_ptr() - flat.data_ptr()) // 4
                assert 0 <= off and off + p.numel() <= flat.numel()                 # the centres live in the arena
                moved = flat[off:off + p.numel()].view_as(p0)
                assert not torch.equal(moved, p0) and bool(torch.isfinite(moved).all())
            return flat.detach().clone(), tr.arena.m.detach().clone(), costs, tr.replayed_steps
        pe, me, ce, _ = run(False)
        pl, ml, cl, replayed = run(True)
        assert replayed > 0 and all(np.isfinite(ce))
        assert torch.equal(pe, pl) and torch.equal(me, ml), float((pe - pl).abs().max())
        assert ce[-len(cl):] == cl, (ce, cl)
    finally:
        ops.CONV_PRECISION = old


def _decode_inputs(dev):
    fc, fp, cc, cp, _ = R.seeded_inputs()
    h = {k: torch.from_numpy(v).to(dev) for k, v in head_outputs().items()}
    h["conf"] = _head(torch.from_numpy(fc).to(dev), torch.from_numpy(cc).to(dev)).permute(0, 2, 1).contiguous()
    h["prop_conf"] = _head(torch.from_numpy(fp).to(dev), torch.from_numpy(cp).to(dev)).permute(0, 2, 1).contiguous()
    return h


def _check_decode(fx, tag, dec):
    assert dec['unct'] is None and dec['actn'] is None
    for ci in range(2):
        np.testing.assert_allclose(dec['seg'][ci].cpu().numpy(), fx[f"{tag}_seg_{ci}"], rtol=1e-6, atol=1e-5)
        np.testing.assert_allclose(dec['score'][ci].cpu().numpy(), fx[f"{tag}_score_{ci}"][1:], rtol=1e-5, atol=1e-7)


@pytest.mark.parametrize("name", ["rpl", "gcpl"])
def test_decode_matches_golden(fx, name):
    """decode_clips(use_gcpl=...) on the fixture's distance maps against the reference's segments and conf_scores; the
    fused RPL run decodes the average of the two samples (tools/pin_rpl.py)."""
    from opental_amd.thumos14 import test as T
    dev = torch.device("cuda", 0)
    clips = fx["clips"]
    offs, fps = list(clips[:, 0]), list(clips[:, 1])
    h = _decode_inputs(dev)
    single = dict(h, priors=priors().to(dev))
    _check_decode(fx, f"dec_{name}_fus0", T.decode_clips(single, offs, fps, os_head=False, use_edl=False, use_gcpl=name == "gcpl"))
    avg = {k: ((v[0] + v[1]) / 2.0).unsqueeze(0).expand(2, *v.shape[1:]).contiguous() for k, v in h.items()}
    avg['priors'] = priors().to(dev)
    if name == "rpl":
        _check_decode(fx, "dec_rpl_fus1", T.decode_clips(avg, offs, fps, os_head=False, use_edl=False))
        return
    # GCPL with fusion.  The reference's parse_output negates the rgb stream only (test.py:85-87 come before the average of
    # :96-99), so its fused scores are the softmax of (flow - rgb) / 2: the golden rows are reproduced by exactly that ...
    quirk = dict(avg)
    for k in ("conf", "prop_conf"):
        quirk[k] = torch.stack([(-h[k][0] + h[k][1]) / 2.0, (-h[k][1] + h[k][0]) / 2.0]).contiguous()    # clip 1: streams swapped
    _check_decode(fx, "dec_gcpl_fus1", T.decode_clips(quirk, offs, fps, os_head=False, use_edl=False))
    # ... while the package negates the AVERAGE of the two streams (both are distances): the softmax of -(rgb + flow) / 2
    a = T.decode_clips(avg, offs, fps, os_head=False, use_edl=False, use_gcpl=True)
    b = T.decode_clips(dict(avg, conf=-avg['conf'], prop_conf=-avg['prop_conf']), offs, fps, os_head=False, use_edl=False)
    assert torch.equal(a['score'], b['score']) and torch.equal(a['flag'], b['flag']) and torch.equal(a['seg'], b['seg'])


def test_fused_gcpl_run_negates_both_streams():
    """detect_batch with a flow network: the decode sees the negated average of the two networks' distance maps."""
    from opental_amd.common import ops
    from opental_amd.thumos14 import test as T
    dev = torch.device("cuda", 0)
    old = ops.CONV_PRECISION
    ops.CONV_PRECISION = 0
    try:
        rgb, flow = rpl_net(3, 0).to(dev).eval(), rpl_net(2, 1).to(dev).eval()
        rgb.use_gcpl = flow.use_gcpl = True
        g = torch.Generator(device=dev).manual_seed(8)
        v = torch.randint(0, 256, (3, 300, 96, 96), device=dev, generator=g, dtype=torch.uint8)
        fv = torch.randint(0, 256, (2, 300, 96, 96), device=dev, generator=g, dtype=torch.uint8)
        rows, counts, _, dec = T.detect_batch(rgb, [v], 10.0, flow_net=flow, flow_videos=[fv])
        offs = T.get_offsets(300, 256, 128)
        w = [(0, o) for o in offs]
        with torch.no_grad():
            fused = T.fuse_outputs(rgb(T.prepare_windows([v], w, 256)), flow(T.prepare_windows([fv], w, 256)))
        neg = dict(fused, conf=-fused['conf'], prop_conf=-fused['prop_conf'])
        ref = T.decode_clips(neg, [float(o) for o in offs], [10.0] * len(offs), os_head=False, use_edl=False)
        assert torch.equal(ref['score'], dec['score']) and torch.equal(ref['flag'], dec['flag'])
        assert int(counts.sum()) > 0
    finally:
        ops.CONV_PRECISION = old


@pytest.fixture
def _restore_precision():
    from opental_amd.common import ops
    old = ops.CONV_PRECISION
    yield
    ops.CONV_PRECISION = old


@pytest.mark.parametrize("name", ["rpl", "gcpl"])
def test_train_test_and_threshold_drivers_on_rpl_configs(tmp_path, name, _restore_precision):
    """The synthetic yaml rewritten to thumos14_open_rpl.yaml / thumos14_open_gcpl.yaml (use_rpl, rpl_loss with its
    rpl_config, no os_head, no use_edl): two training steps, the test driver with the 'confidence' open-set evaluation, and
    the threshold driver with --ood_scoring confidence."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    from make_synthetic_thumos import make
    from opental_amd.thumos14 import train as TR, test as T, threshold as TH
    src = make(str(tmp_path / "data"), videos=2, frames=400, size=100)
    cfg = yaml.load(open(src).read(), Loader=yaml.FullLoader)
    md, tr = cfg['model'], cfg['training']
    md.pop('os_head', None)
    md.pop('use_edl', None)
    md['use_rpl'] = True
    tr.pop('act_config', None)
    tr.pop('edl_config', None)
    tr['edl_loss'], tr['focal_loss'], tr['rpl_loss'] = False, False, True
    tr['rpl_config'] = dict(VARIANTS[name])
    cfg['testing']['ood_scoring'] = 'confidence'
    path = str(tmp_path / f"{name}.yaml")
    with open(path, "w") as f:
        yaml.dump(cfg, f)
    flags = ['--open_set', '--split', '0', '--lw', '1', '--cw', '10', '--piou', '0.5', '--ssl', '0.001', '--batch_size', '2']
    trainer, hist = TR.main([path] + flags + ['--random_init', '--save_after', '0', '--max_steps', '2', '--max_epoch', '1',
                                              '--checkpoint_path', str(tmp_path / "run")])
    assert not trainer.net.os_head and trainer.net.use_rpl and trainer.criterion.cls_loss_type == 'rpl'
    assert bool(trainer.criterion.cls_loss.gcpl) == (name == "gcpl")
    assert trainer.step_count == 2 and all(np.isfinite(h).all() for h in hist)
    known = tmp_path / "known.txt"
    known.write_text(open(tmp_path / "data" / "classes.txt").read())
    out_file, metrics = T.main([path, '--open_set', '--split', '0', '--checkpoint_path', str(tmp_path / "run" / "checkpoint-1.ckpt"),
                                '--evaluate', str(tmp_path / "data" / "gt_open.json"), str(known)])
    res = json.load(open(out_file))
    assert res['version'] == 'THUMOS14' and len(res['results']) == 2
    props = [p for v in res['results'].values() for p in v]
    assert props
    for p in props[:200]:
        assert set(p) == {'label', 'score', 'segment', 'uncertainty', 'actionness'} and len(p['segment']) == 2
        assert p['actionness'] == 0.0 and p['uncertainty'] == 0.0
    assert metrics is None or all(np.isfinite(np.asarray(v)).all() for v in metrics.values())
    th_file, thr = TH.main([path, '--open_set', '--split', '0', '--random_init', '--ood_scoring', 'confidence',
                            '--output_json', 'thresh.json'])
    th = json.load(open(th_file))
    tprops = [p for v in th['results'].values() for p in v]
    assert tprops and all(p['uncertainty'] == 0.0 and p['actionness'] == 0.0 for p in tprops[:200])
    assert th['external_data']['threshold'] == thr and np.isfinite(thr)
