"""GPU: the closed-set Softmax and EDL baselines (os_head false) -- fused loss modes 2 / 3, otal_decode_clips_ex, the
batched inference path with and without two-stream fusion, the model forward, the captured training step and the train /
test drivers -- against tests/golden/closed_set.npz (tools/pin_closed_set.py) and the package's own host formulations."""
import json
import os
import sys

import numpy as np
import pytest
import torch
import yaml

from oracle import arch

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C = 16
EDL_CFG = dict(evidence='exp', loss_type='log', soft_label=0, with_focal=False, alpha=0.25, gamma=2)
W = dict(lw=1.0, cw=10.0, ctw=1.0, actw=1.0, ssl=0.001)


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "closed_set.npz"))


def head_outputs(B=2, seed=31):
    """The synthetic head outputs of tools/pin_closed_set.py (same seed, same draws)."""
    rs = np.random.RandomState(seed)
    K = sum(arch.level_lengths())
    return dict(loc=rs.uniform(2.0, 40.0, (B, K, 2)).astype(np.float32),
                conf=rs.normal(0.0, 2.0, (B, K, C)).astype(np.float32),
                prop_loc=rs.normal(0.0, 0.3, (B, K, 2)).astype(np.float32),
                prop_conf=rs.normal(0.0, 2.0, (B, K, C)).astype(np.float32),
                center=rs.normal(0.0, 1.0, (B, K, 1)).astype(np.float32))


def priors(dev):
    return torch.tensor([[(c + 0.5) / t] for t in arch.level_lengths() for c in range(t)], dtype=torch.float32, device=dev)


def closed_set_params(seed=2020, head_seed=4242):
    """tools/pin_closed_set.py closed_set_params: arch.make_params without the actionness heads, 16-class conf heads."""
    p = {k: v for k, v in arch.make_params(seed).items() if "actionness_head" not in k}
    rs = np.random.RandomState(head_seed)
    for head, k in (("conf_head", 3), ("prop_conf_head", 1)):
        key = f"coarse_pyramid_detection.{head}.conv1d"
        lim = np.sqrt(3.0 / max(1.0, (512 * k + C * k) / 2.0))
        p[key + ".weight"] = rs.uniform(-lim, lim, size=(C, 512, k)).astype(np.float32)
        p[key + ".bias"] = rs.uniform(-0.1, 0.1, size=(C,)).astype(np.float32)
    return p


def closed_net(use_edl=True, in_channels=3, seed=0):
    from opental_amd.thumos14.BDNet import BDNet, DEFAULT_MODEL_CFG
    torch.manual_seed(seed)
    net = BDNet(in_channels=in_channels, training=False, use_edl=use_edl, cfg=dict(DEFAULT_MODEL_CFG, os_head=False))
    net.backbone._model.apply(BDNet.weight_init)
    return net


def _criterion(kind, dev):
    from opental_amd.thumos14 import multisegment_loss as M
    return M.MultiSegmentLoss(C, 0.5, 1.0, cls_loss_type=kind, edl_config=EDL_CFG if kind == 'edl' else None,
                              os_head=False).to(dev)


def _run_loss(kind, fused, out_np, targets, dev):
    from opental_amd.thumos14 import multisegment_loss as M
    M.FUSED = fused
    try:
        crit = _criterion(kind, dev)
        ins = {k: torch.from_numpy(v).to(dev).requires_grad_(True) for k, v in out_np.items()}
        losses = crit(dict(ins, priors=priors(dev), act=None, prop_act=None), targets)
        assert ('DetectionLossFunction' in type(losses[0].grad_fn).__name__) == fused
        assert losses[5] is None and losses[6] is None
        sum(l * w for l, w in zip(losses[:5], (1.0, 10.0, 1.0, 10.0, 1.0))).backward()
        return [float(l.detach()) for l in losses[:5]], {k: v.grad.clone() for k, v in ins.items()}
    finally:
        M.FUSED = True


@pytest.mark.parametrize("kind", ["focal", "edl"])
def test_fused_closed_set_loss_matches_golden(fx, kind):
    dev = torch.device("cuda", 0)
    targets = [torch.from_numpy(fx["targets_0"]).to(dev), torch.from_numpy(fx["targets_1"]).to(dev)]
    terms, grads = _run_loss(kind, True, head_outputs(), targets, dev)
    assert np.allclose(terms, fx[f"loss_{kind}_terms"], rtol=2e-5, atol=1e-6), (terms, fx[f"loss_{kind}_terms"])
    for k, g in grads.items():
        ref = torch.from_numpy(fx[f"loss_{kind}_grad_{k}"]).to(dev)
        scale = float(ref.abs().max())
        assert float((g - ref).abs().max()) <= 2e-5 * max(scale, 1e-6), k


@pytest.mark.parametrize("kind", ["focal", "edl"])
@pytest.mark.parametrize("B", [1, 2, 8, 16])
def test_fused_closed_set_loss_matches_torch_formulation(kind, B):
    dev = torch.device("cuda", 0)
    rs = np.random.RandomState(B)
    out_np = head_outputs(B, seed=100 + B)
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
    l0, g0 = _run_loss(kind, False, out_np, targets, dev)
    l1, g1 = _run_loss(kind, True, out_np, targets, dev)
    assert np.allclose(l0, l1, rtol=2e-5, atol=1e-6), (l0, l1)
    for k in g0:
        scale = float(g0[k].abs().max())
        assert scale > 0, k
        assert float((g0[k] - g1[k]).abs().max()) <= 2e-5 * scale, (k, scale)


def _decode_ex(out, offsets, fps, score_fn, first_class, act=None, conf_thresh=0.01):
    from opental_amd import _lib as L
    t = lambda k: out[k].contiguous()
    n, A, _ = out['loc'].shape
    K = out['conf'].shape[-1]
    dev = out['loc'].device
    seg = torch.empty(n, A, 2, device=dev)
    score = torch.empty(n, K - first_class, A, device=dev)
    unct, actn = torch.empty(n, A, device=dev), torch.empty(n, A, device=dev)
    flag = torch.empty(n, K - first_class, A, dtype=torch.uint8, device=dev)
    offs = torch.tensor(offsets, dtype=torch.float32, device=dev)
    fpst = torch.tensor(fps, dtype=torch.float32, device=dev)
    p = lambda v: None if v is None else L.ptr(v)
    L.check(L.lib().otal_decode_clips_ex(L.ptr(t('loc')), L.ptr(t('prop_loc')), L.ptr(out['priors'].contiguous()),
                                         L.ptr(t('conf')), L.ptr(t('prop_conf')), L.ptr(t('center')),
                                         p(None if act is None else act[0]), p(None if act is None else act[1]),
                                         L.ptr(offs), L.ptr(fpst), L.ptr(seg), L.ptr(score), L.ptr(unct), L.ptr(actn),
                                         L.ptr(flag), n, A, K, 256.0, conf_thresh,
                                         score_fn, first_class, L.stream()), "otal_decode_clips_ex")
    return seg, score, unct, actn, flag


def _outputs(dev, fusion):
    h = {k: torch.from_numpy(v).to(dev) for k, v in head_outputs().items()}
    if fusion:      # both clips decode the average of the two samples (tools/pin_closed_set.py)
        h = {k: ((v[0] + v[1]) / 2.0).unsqueeze(0).expand(2, *v.shape[1:]).contiguous() for k, v in h.items()}
    h['priors'] = priors(dev)
    return h


@pytest.mark.parametrize("use_edl", [False, True])
@pytest.mark.parametrize("fusion", [False, True])
def test_decode_ex_matches_golden(fx, use_edl, fusion):
    """The bounds of test_infer_gpu.py::test_decode_and_filter_golden; the flags equal the reference's masks exactly."""
    dev = torch.device("cuda", 0)
    tag = f"dec_edl{int(use_edl)}_fus{int(fusion)}"
    out = _outputs(dev, fusion)
    clips = fx["clips"]
    seg, score, unct, _, flag = _decode_ex(out, list(clips[:, 0]), list(clips[:, 1]), 0 if use_edl else 1, 1)
    for ci in range(2):
        np.testing.assert_allclose(seg[ci].cpu().numpy(), fx[f"{tag}_seg_{ci}"], rtol=1e-6, atol=1e-5)
        np.testing.assert_allclose(score[ci].cpu().numpy(), fx[f"{tag}_score_{ci}"][1:], rtol=1e-5, atol=1e-7)
        if use_edl and not fusion:      # (a fused run's uncertainty is the average of the networks' own maps)
            np.testing.assert_allclose(unct[ci].cpu().numpy(), fx[f"{tag}_unct_{ci}"], rtol=1e-5, atol=1e-7)
        assert np.array_equal(flag[ci].cpu().numpy(), fx[f"{tag}_mask_{ci}"][1:])


def test_decode_entry_is_the_ex_entry_with_the_opental_head():
    from opental_amd import _lib as L
    from opental_amd.thumos14.test import decode_clips
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(3)
    n, A, K = 5, 126, 15
    out = dict(loc=torch.rand(n, A, 2, generator=g) * 30 + 1, prop_loc=torch.randn(n, A, 2, generator=g) * 0.3,
               conf=torch.randn(n, A, K, generator=g) * 6, prop_conf=torch.randn(n, A, K, generator=g) * 6,
               center=torch.randn(n, A, 1, generator=g), act=torch.randn(n, A, 1, generator=g) * 2,
               prop_act=torch.randn(n, A, 1, generator=g) * 2)
    out = {k: v.to(dev) for k, v in out.items()}
    out['priors'] = priors(dev)
    offs, fps = [0.0, 128.0, 256.0, 384.0, 512.0], [10.0, 25.0, 30.0, 10.0, 12.5]
    a = decode_clips(out, offs, fps)
    b = _decode_ex(out, offs, fps, 0, 0, act=(out['act'], out['prop_act']))
    for k, v in zip(('seg', 'score', 'unct', 'actn', 'flag'), b):
        assert torch.equal(a[k], v), k


def _host_detections(net_out, offsets, fps, use_edl, fused_unct=False, top_k=5000, sigma=0.5, conf_thresh=0.01):
    """Per clip decode_predictions + filtering, then segment_utils.softnms_v2 per class: the reference's loop
    (test.py:203-244) for one video.  fused_unct: the uncertainty is the average of the networks' own maps."""
    from opental_amd.common.segment_utils import softnms_v2
    from opental_amd.thumos14 import test as T
    output = [[] for _ in range(C - 1)]
    for i, off in enumerate(offsets):
        seg, score, unct, actn = T.decode_predictions(net_out, i, float(off), fps, 256, os_head=False, use_edl=use_edl)
        assert actn is None and (unct is None) != use_edl
        if fused_unct:
            unct = (net_out['unct'][i] + net_out['prop_unct'][i]) / 2.0
        for cl in range(C - 1):
            rows = T.filtering(seg, score[cl], unct, actn, conf_thresh, use_edl=use_edl, os_head=False)
            if rows is not None:
                assert rows.shape[1] == 3 + use_edl
                output[cl].append(rows)
    res = {}
    for cl in range(C - 1):
        if output[cl]:
            rows, cnt = softnms_v2(torch.cat(output[cl], 0), sigma=sigma, top_k=top_k, score_threshold=0.001,
                                   use_edl=use_edl, os_head=False)[:2]
            res[cl] = rows[:int(cnt)].cpu()
    return res


def _compare_batch(rows, counts, host, use_edl):
    cols = 3 + use_edl
    assert rows.shape[-1] == cols
    for cl in range(C - 1):
        cnt = int(counts[cl])
        want = host.get(cl, torch.zeros(0, cols))
        assert cnt == want.shape[0], (cl, cnt, want.shape)
        if cnt:
            np.testing.assert_allclose(rows[cl, :cnt].cpu().numpy(), want.numpy(), rtol=2e-6, atol=1e-7)


@pytest.mark.parametrize("use_edl", [False, True])
def test_detect_batch_closed_set_matches_host_path(use_edl):
    from opental_amd.common import ops
    from opental_amd.thumos14 import test as T
    dev = torch.device("cuda", 0)
    old = ops.CONV_PRECISION
    ops.CONV_PRECISION = 0
    try:
        net = closed_net(use_edl).to(dev).eval()
        g = torch.Generator(device=dev).manual_seed(7)
        video = torch.randint(0, 256, (3, 400, 96, 96), device=dev, generator=g, dtype=torch.uint8)
        rows, counts, _, dec = T.detect_batch(net, [video], 10.0, conf_thresh=0.01)
        assert dec['actn'] is None and (dec['unct'] is None) != use_edl
        offs = T.get_offsets(400, 256, 128)
        with torch.no_grad():
            out = net(T.prepare_windows([video], [(0, o) for o in offs], 256))
        _compare_batch(rows[0], counts[0], _host_detections(out, offs, 10.0, use_edl), use_edl)
        props = T.get_video_detections(rows[0], counts[0], {i: f"c{i}" for i in range(1, C)}, 5000)
        assert props and all(p['actionness'] == 0.0 for p in props)
    finally:
        ops.CONV_PRECISION = old


@pytest.mark.parametrize("use_edl", [False, True])
def test_closed_set_fusion_decodes_the_averaged_outputs(use_edl):
    from opental_amd.common import ops
    from opental_amd.thumos14 import test as T
    dev = torch.device("cuda", 0)
    old = ops.CONV_PRECISION
    ops.CONV_PRECISION = 0
    try:
        rgb, flow = closed_net(use_edl, 3, 0).to(dev).eval(), closed_net(use_edl, 2, 1).to(dev).eval()
        g = torch.Generator(device=dev).manual_seed(8)
        v = torch.randint(0, 256, (3, 300, 96, 96), device=dev, generator=g, dtype=torch.uint8)
        fv = torch.randint(0, 256, (2, 300, 96, 96), device=dev, generator=g, dtype=torch.uint8)
        rows, counts, _, dec = T.detect_batch(rgb, [v], 10.0, flow_net=flow, flow_videos=[fv])
        offs = T.get_offsets(300, 256, 128)
        w = [(0, o) for o in offs]
        with torch.no_grad():
            fused = T.fuse_outputs(rgb(T.prepare_windows([v], w, 256)), flow(T.prepare_windows([fv], w, 256)))
        ref = T.decode_clips(fused, [float(o) for o in offs], [10.0] * len(offs), os_head=False, use_edl=use_edl)
        assert torch.equal(ref['score'], dec['score']) and torch.equal(ref['flag'], dec['flag'])
        if use_edl:
            assert torch.equal(dec['unct'], (fused['unct'] + fused['prop_unct']) / 2.0)
        _compare_batch(rows[0], counts[0], _host_detections(fused, offs, 10.0, use_edl, fused_unct=use_edl), use_edl)
        with pytest.raises(RuntimeError):
            T.detect_batch(rgb, [v], 10.0, flow_net=closed_net(not use_edl, 2).to(dev).eval(), flow_videos=[fv])
    finally:
        ops.CONV_PRECISION = old


def test_closed_set_model_forward_matches_golden(fx):
    from opental_amd.common import ops
    from opental_amd.thumos14.BDNet import BDNet, DEFAULT_MODEL_CFG
    dev = torch.device("cuda", 0)
    old = ops.CONV_PRECISION
    ops.CONV_PRECISION = 0
    try:
        net = BDNet(training=False, use_edl=True, cfg=dict(DEFAULT_MODEL_CFG, os_head=False))
        params = closed_set_params(int(fx["model_param_seed"]), int(fx["model_head_seed"]))
        net.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
        net = net.to(dev).eval()
        x = torch.from_numpy(arch.make_clip(int(fx["model_clip_seed"]), 1)).to(dev)
        with torch.no_grad():
            out = net(x)
        assert out['act'] is None and out['prop_act'] is None
        rel = lambda a, b: float(np.abs(np.asarray(a, np.float64) - b).max() / max(np.abs(b).max(), 1e-6))
        for k in ("loc", "conf", "prop_loc", "prop_conf", "center", "unct", "prop_unct"):
            assert rel(out[k].cpu().numpy(), fx[f"model_out_{k}"]) < 1e-4, k
        for k in ("start", "end", "start_loc_prop", "end_loc_prop", "start_conf_prop", "end_conf_prop"):
            f = out[k].detach().reshape(-1)
            assert rel(f[::max(1, f.numel() // 1024)].cpu().numpy(), fx[f"model_probe_{k}"]) < 1e-4, k
    finally:
        ops.CONV_PRECISION = old


@pytest.mark.parametrize("kind", ["focal", "edl"])
def test_closed_set_lane_graph_steps_equal_eager_steps(kind):
    """A closed-set model and criterion through DetectorTrainer: the capture's warm-up step plus three replayed lane-graph
    steps leave parameters and Adam moments BIT-IDENTICAL to four eager steps."""
    import bench
    from opental_amd.common import ops
    from opental_amd.thumos14.train import DetectorTrainer
    dev = torch.device("cuda", 0)
    old = ops.CONV_PRECISION
    ops.CONV_PRECISION = 1
    try:
        clips, targets, scores = bench.synth_batch(2, 1000, dev)

        def run(lanes):
            net = closed_net(kind == 'edl', seed=5).to(dev).train()
            tr = DetectorTrainer(net, _criterion(kind, dev), W, lr=1e-4, weight_decay=1e-3)
            done = 0
            if lanes:
                tr.capture_step(clips, targets, scores, warmup=1, lanes=True)       # the warm-up step is a real step
                assert tr._graph[0] == "lanes"
                done = 1
            costs = [float(tr.step(clips, targets, scores)[0]) for _ in range(4 - done)]
            torch.cuda.synchronize()
            assert tr.step_count == 4
            return tr.arena.flat.detach().clone(), tr.arena.m.detach().clone(), costs, tr.replayed_steps
        pe, me, ce, _ = run(False)
        pl, ml, cl, replayed = run(True)
        assert replayed > 0 and all(np.isfinite(ce))
        assert torch.equal(pe, pl) and torch.equal(me, ml), float((pe - pl).abs().max())
        assert ce[-len(cl):] == cl, (ce, cl)
    finally:
        ops.CONV_PRECISION = old


@pytest.fixture
def _restore_precision():
    from opental_amd.common import ops
    old = ops.CONV_PRECISION
    yield
    ops.CONV_PRECISION = old


@pytest.mark.parametrize("baseline", ["softmax", "edl"])
def test_train_and_test_drivers_on_closed_set_configs(tmp_path, baseline, _restore_precision):
    """The synthetic yaml rewritten to the Softmax baseline (thumos14_softmax.yaml: focal loss, no os_head, no use_edl)
    and to the EDL baseline (thumos14_open_edl.yaml: edl_loss with its edl_config, use_edl, no os_head); two training
    steps, the test driver and the 'confidence' open-set evaluation of its result file."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    from make_synthetic_thumos import make
    from opental_amd.thumos14 import train as R, test as T
    src = make(str(tmp_path / "data"), videos=2, frames=400, size=100)
    cfg = yaml.load(open(src).read(), Loader=yaml.FullLoader)
    md, tr = cfg['model'], cfg['training']
    md.pop('os_head', None)
    tr.pop('act_config', None)
    if baseline == "softmax":
        md.pop('use_edl', None)
        tr['edl_loss'], tr['focal_loss'] = False, True
        tr.pop('edl_config', None)
    else:
        md['use_edl'], md['evidence'] = True, 'exp'
        tr['edl_loss'], tr['focal_loss'] = True, False
        tr['edl_config'] = dict(EDL_CFG)
    cfg['testing']['ood_scoring'] = 'confidence'
    path = str(tmp_path / f"{baseline}.yaml")
    with open(path, "w") as f:
        yaml.dump(cfg, f)
    flags = ['--open_set', '--split', '0', '--lw', '1', '--cw', '10', '--piou', '0.5', '--ssl', '0.001', '--batch_size', '2']
    trainer, hist = R.main([path] + flags + ['--random_init', '--save_after', '0', '--max_steps', '2', '--max_epoch', '1',
                                             '--checkpoint_path', str(tmp_path / "run")])
    assert not trainer.net.os_head and trainer.criterion.cls_loss_type == ('focal' if baseline == 'softmax' else 'edl')
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
        assert p['actionness'] == 0.0 and (p['uncertainty'] == 0.0) == (baseline == 'softmax')
    assert metrics is None or all(np.isfinite(np.asarray(v)).all() for v in metrics.values())
