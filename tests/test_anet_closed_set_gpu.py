"""GPU: the ActivityNet1.3 closed-set Softmax and EDL baselines (os_head false) -- fused loss modes 2 / 3 of
otal_detection_loss_anet_ex, the model forward with 151-class heads, decode + Soft-NMS, detect_batch, the captured training
step and the train / test drivers -- against tests/golden/anet_closed_set.npz (tools/pin_anet_closed_set.py) and the
package's own host formulations."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch
import yaml

from oracle import afsd_oracle as O
from oracle import arch

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C = 151
EDL_CFG = dict(evidence='exp', loss_type='log')
W = dict(lw=1.0, cw=1.0, ctw=1.0, actw=1.0, ssl=0.1)
BASE_FLAGS = ['--open_set', '--split', '0', '--lw', '1', '--cw', '1', '--piou', '0.6']


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "anet_closed_set.npz"))


def head_outputs(seed=57, batch=2, center_mean=0.0):
    """tools/pin_anet_closed_set.py head_outputs: the same seed, the same draws."""
    rs = np.random.RandomState(seed)
    pri = O.priors_all(arch.ANET).numpy()
    K = pri.shape[0]
    stride = np.array([arch.ANET["fpn_strides"][int(l)] for l in pri[:, 1]], np.float32)
    return dict(loc=(rs.uniform(0.5, 6.0, (batch, K, 2)) * stride[None, :, None]).astype(np.float32),
                conf=rs.normal(0.0, 2.0, (batch, K, C)).astype(np.float32),
                prop_loc=rs.normal(0.0, 0.3, (batch, K, 2)).astype(np.float32),
                prop_conf=rs.normal(0.0, 2.0, (batch, K, C)).astype(np.float32),
                center=rs.normal(center_mean, 1.0, (batch, K, 1)).astype(np.float32))


def closed_set_params(seed=2020, head_seed=5151):
    """tools/pin_anet_closed_set.py closed_set_params: arch.make_params(ANET) without the actionness heads, 151-class conf
    heads."""
    p = {k: v for k, v in arch.make_params(seed, arch.ANET).items() if "actionness_head" not in k}
    rs = np.random.RandomState(head_seed)
    for head, k in (("conf_head", 3), ("prop_conf_head", 1)):
        key = f"coarse_pyramid_detection.{head}.conv1d"
        lim = np.sqrt(3.0 / max(1.0, (512 * k + C * k) / 2.0))
        p[key + ".weight"] = rs.uniform(-lim, lim, size=(C, 512, k)).astype(np.float32)
        p[key + ".bias"] = rs.uniform(-0.1, 0.1, size=(C,)).astype(np.float32)
    return p


def closed_net(use_edl=True, seed=0):
    from opental_amd.anet.BDNet import BDNet, DEFAULT_MODEL_CFG
    torch.manual_seed(seed)
    net = BDNet(training=False, use_edl=use_edl, cfg=dict(DEFAULT_MODEL_CFG, os_head=False))
    net.backbone._model.apply(BDNet.weight_init)
    return net


def strided(t, n=4096):
    f = t.detach().reshape(-1)
    return f[::max(1, f.numel() // n)]


def _criterion(kind, dev, iou_aware=False):
    from opental_amd.anet import multisegment_loss as M
    cfg = dict(EDL_CFG, iou_aware=True) if iou_aware else EDL_CFG
    return M.MultiSegmentLoss(C, 0.6, 1.0, cls_loss_type=kind, edl_config=cfg if kind == 'edl' else None,
                              os_head=False).to(dev)


def _run_loss(kind, fused, out_np, targets, dev, weights=(1.0,) * 5, iou_aware=False):
    from opental_amd.anet import multisegment_loss as M
    M.FUSED = fused
    try:
        crit = _criterion(kind, dev, iou_aware)
        ins = {k: torch.from_numpy(v).to(dev).requires_grad_(True) for k, v in out_np.items()}
        pri = O.priors_all(arch.ANET).to(dev)
        losses = crit([ins["loc"], ins["conf"], ins["prop_loc"], ins["prop_conf"], ins["center"], pri, None, None], targets)
        assert ('AnetDetectionLossFunction' in type(losses[0].grad_fn).__name__) == fused
        assert losses[5] is None and losses[6] is None
        sum(l * w for l, w in zip(losses[:5], weights)).backward()
        return np.array([float(l.detach()) for l in losses[:5]]), {k: v.grad.clone() for k, v in ins.items()}
    finally:
        M.FUSED = True


@pytest.mark.parametrize("kind", ["focal", "edl"])
def test_fused_closed_set_loss_matches_golden(fx, kind):
    """cls_mode 3 (focal) and 2 (EDL) of otal_detection_loss_anet_ex against the reference's terms and gradients."""
    dev = torch.device("cuda", 0)
    targets = [torch.from_numpy(fx["targets_0"]).to(dev), torch.from_numpy(fx["targets_1"]).to(dev)]
    terms, grads = _run_loss(kind, True, head_outputs(), targets, dev, tuple(fx["weights"]))
    assert np.allclose(terms, fx[f"loss_{kind}_terms"], rtol=2e-5, atol=1e-6), (terms, fx[f"loss_{kind}_terms"])
    for k, g in grads.items():
        ref = torch.from_numpy(fx[f"loss_{kind}_grad_{k}"]).to(dev)
        scale = float(ref.abs().max())
        assert float((strided(g) - ref).abs().max()) <= 2e-5 * max(scale, 1e-6), k


def _case_targets(case, dev):
    """The target sets of tests/test_anet_gpu.py::test_fused_anet_loss_equals_the_torch_formulation."""
    def seg(a, b, lab):
        return [a / 768.0, b / 768.0, float(lab)]
    if case == "single_positive_level":
        targets = [np.array([seg(100, 140, 5)], np.float32), np.array([seg(300, 330, 9), seg(500, 540, 2)], np.float32),
                   np.array([seg(20, 60, 150)], np.float32)]
    else:
        targets = [np.array([seg(50, 250, 3), seg(400, 430, 17), seg(600, 760, 150), seg(300, 320, 1)], np.float32),
                   np.array([seg(10, 700, 42)], np.float32),
                   np.array([seg(200, 260, 7), seg(220, 500, 8)], np.float32)]
    if case == "no_targets_in_one_sample":
        targets[1] = np.zeros((0, 3), np.float32)
    return [torch.from_numpy(t).to(dev) for t in targets]


@pytest.mark.parametrize("kind", ["focal", "edl", "edl_iou_aware"])
@pytest.mark.parametrize("case", ["mixed", "no_targets_in_one_sample", "single_positive_level", "other_draw"])
def test_fused_closed_set_loss_matches_torch_formulation(kind, case):
    """Fused modes 2 / 3 against this package's torch formulation (itself pinned to the reference): the five terms to 2e-5
    and the gradient of a weighted sum w.r.t. every head output to 2e-5 of its scale.  EDL also with the IoU calibration
    (u = C / S over the 151 logits)."""
    dev = torch.device("cuda", 0)
    seed = {"mixed": 1, "no_targets_in_one_sample": 2, "single_positive_level": 3, "other_draw": 4}[case]
    targets = _case_targets(case, dev)
    out_np = head_outputs(seed=100 + seed, batch=3)
    weights = (1.0, 0.7, 1.3, 0.9, 1.1)
    k, iou = ("edl", True) if kind == "edl_iou_aware" else (kind, False)
    t0, g0 = _run_loss(k, False, out_np, targets, dev, weights, iou)
    t1, g1 = _run_loss(k, True, out_np, targets, dev, weights, iou)
    assert np.isfinite(t1).all()
    assert (np.abs(t1 - t0) <= 2e-5 * np.maximum(1.0, np.abs(t0))).all(), (t1, t0)
    for name in g0:
        scale = float(g0[name].abs().max())
        assert scale > 0, name
        assert float((g0[name] - g1[name]).abs().max()) <= 2e-5 * scale + 1e-9, (name, scale)


def test_ex_mode_0_is_the_opental_entry_bit_for_bit():
    """otal_detection_loss_anet == otal_detection_loss_anet_ex(cls_mode 0): the same seven terms and gradient buffer, bitwise
    (IBM weight and IoU calibration on); the closed-set modes write 0 to terms 5 / 6 and to their gradient slots."""
    from opental_amd import _lib as L
    from opental_amd.anet.multisegment_loss import bounds
    dev = torch.device("cuda", 0)
    rs = np.random.RandomState(9)
    B, Cw = 3, 150
    out = head_outputs(seed=11, batch=B)
    t = {k: torch.from_numpy(v).to(dev) for k, v in out.items()}
    conf, pconf = t["conf"][..., :Cw].contiguous(), t["prop_conf"][..., :Cw].contiguous()
    act = torch.from_numpy(rs.randn(B, 189).astype(np.float32)).to(dev)
    pact = torch.from_numpy(rs.randn(B, 189).astype(np.float32)).to(dev)
    pri = O.priors_all(arch.ANET).to(dev).contiguous()
    tg = _case_targets("mixed", dev)
    from opental_amd.thumos14.multisegment_loss import as_padded
    gt, valid = as_padded(tg, dev)
    gt, gv = gt.contiguous(), valid.contiguous().to(torch.uint8)
    lib = L.lib()
    lbs = (ctypes.c_float * 12)(*[float(v) for row in bounds for v in row])

    def run(ex, mode=0, a=act, pa=pact, cf=conf, pcf=pconf):
        Cc = cf.shape[-1]
        ng = lib.otal_detection_loss_grad_floats(B, 189, Cc)
        losses = torch.full((7,), float('nan'), device=dev)
        grads = torch.full((ng,), float('nan'), device=dev)
        scratch = torch.empty(8 * B, device=dev)
        args = [L.ptr(t["loc"]), L.ptr(cf), L.ptr(t["prop_loc"]), L.ptr(pcf), L.ptr(t["center"]),
                None if a is None else L.ptr(a), None if pa is None else L.ptr(pa), L.ptr(pri), L.ptr(gt), L.ptr(gv),
                B, 189, Cc, gt.shape[1], 768.0, 0.6, lbs, 6, int(mode == 0), 10.0, int(mode != 3), 0.1, 1.0]
        if ex:
            rc = lib.otal_detection_loss_anet_ex(*args, mode, 0.25, L.ptr(losses), L.ptr(grads), L.ptr(scratch), L.stream())
        else:
            rc = lib.otal_detection_loss_anet(*args, L.ptr(losses), L.ptr(grads), L.ptr(scratch), L.stream())
        L.check(rc, "loss")
        torch.cuda.synchronize()
        return losses.cpu(), grads.cpu()
    l0, g0 = run(False)
    l1, g1 = run(True)
    assert torch.isfinite(l0).all() and torch.isfinite(g0).all()
    assert torch.equal(l0.view(torch.int32), l1.view(torch.int32)) and torch.equal(g0.view(torch.int32), g1.view(torch.int32))
    A = B * 189
    for mode in (2, 3):
        lm, gm = run(True, mode, None, None, t["conf"], t["prop_conf"])
        assert torch.isfinite(lm).all() and torch.isfinite(gm).all(), mode
        assert float(lm[5]) == 0.0 and float(lm[6]) == 0.0
        assert float(gm[-2 * A:].abs().max()) == 0.0            # dact | dprop_act


def test_closed_set_model_forward_matches_golden(fx):
    """The 151-class conf heads (k = 3 and k = 1, odd Cout) and the absent actionness heads through CoarsePyramid.forward
    and the head tails, fp32, against the reference BDNet with os_head False at b = 1."""
    from opental_amd.common import ops
    from opental_amd.anet.BDNet import BDNet, DEFAULT_MODEL_CFG
    dev = torch.device("cuda", 0)
    old = ops.CONV_PRECISION
    ops.CONV_PRECISION = 0
    try:
        net = BDNet(training=False, use_edl=True, cfg=dict(DEFAULT_MODEL_CFG, os_head=False))
        params = closed_set_params(int(fx["model_param_seed"]), int(fx["model_head_seed"]))
        net.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
        net = net.to(dev).eval()
        x = torch.from_numpy(arch.make_clip(int(fx["model_clip_seed"]), 1, frames=768)).to(dev)
        with torch.no_grad():
            out = net(x)
        assert out['act'] is None and out['prop_act'] is None and tuple(out['conf'].shape) == (1, 189, C)
        rel = lambda a, b: float(np.abs(np.asarray(a, np.float64) - b).max() / max(np.abs(b).max(), 1e-6))
        for k in ("loc", "prop_loc", "center", "unct", "prop_unct"):
            assert rel(out[k].cpu().numpy(), fx[f"model_out_{k}"]) < 1e-4, k
        for k in ("conf", "prop_conf"):
            assert rel(strided(out[k]).cpu().numpy(), fx[f"model_probe_{k}"]) < 1e-4, k
            assert rel(out[k].double().sum(-1).cpu().numpy(), fx[f"model_rowsum_{k}"]) < 1e-4, k
        for k in ("start", "end", "start_loc_prop", "end_loc_prop", "start_conf_prop", "end_conf_prop"):
            f = out[k].detach().reshape(-1)
            assert rel(f[::max(1, f.numel() // 1024)].cpu().numpy(), fx[f"model_probe_{k}"]) < 1e-4, k
    finally:
        ops.CONV_PRECISION = old


VIDEOS = ((61, 25.0, 29.7), (62, 6.0, 120.0))


@pytest.mark.parametrize("use_edl", [False, True])
def test_decode_and_softnms_match_golden(fx, use_edl):
    """decode_clips (otal_decode_clips_ex: softmax / Dirichlet scores, background dropped, no actionness) + Soft-NMS +
    get_video_prediction against the reference's decode_prediction / filtering / get_video_prediction."""
    from opental_amd.anet import test as A
    from opental_amd.thumos14.test import softnms_classes
    dev = torch.device("cuda", 0)
    conf_thresh, top_k, sigma = (float(v) for v in fx["decode_params"])
    heads = [head_outputs(seed, 1, center_mean=-3.0) for seed, _, _ in VIDEOS]
    merged = {k: torch.from_numpy(np.concatenate([h[k] for h in heads], 0)).to(dev) for k in heads[0]}
    merged["priors"] = O.priors_all(arch.ANET).to(dev)
    dec = A.decode_clips(merged, [fps for _, fps, _ in VIDEOS], conf_thresh=conf_thresh, os_head=False, use_edl=use_edl)
    assert dec['actn'] is None and (dec['unct'] is None) == (not use_edl) and dec['score'].shape[1] == C - 1
    rows, counts, _ = softnms_classes(dec, [0, 1, 2], int(top_k), sigma)
    assert rows.shape[-1] == 3 + use_edl
    names = {i: f"class_{i:03d}" for i in range(1, C)}
    for v, (_, fps, duration) in enumerate(VIDEOS):
        tag = f"dec_edl{int(use_edl)}_{v}"
        seg = dec['seg'][v].cpu().numpy()
        assert np.abs(seg - fx[f"{tag}_seg"] / fps).max() < 1e-4 * max(1.0, np.abs(fx[f"{tag}_seg"] / fps).max())
        score = dec['score'][v]
        assert float(np.abs(strided(score, 2048).cpu().numpy() - fx[f"{tag}_score_probe"]).max()) < 1e-6
        assert int(dec['flag'][v].sum()) == int(fx[f"{tag}_nflag"])
        if use_edl:
            assert np.abs(dec['unct'][v].cpu().numpy() - fx[f"{tag}_unct"]).max() < 1e-6
        got = A.get_video_prediction(rows[v], counts[v], duration, names)
        want = fx[f"{tag}_detections"]
        assert len(got) == len(want) > 0, tag
        assert [int(p['label'].split('_')[1]) for p in got] == want[:, 0].astype(int).tolist(), tag
        have = np.array([[p['score'], p['segment'][0], p['segment'][1], p['uncertainty'], p['actionness']] for p in got])
        assert np.abs(have - want[:, 1:]).max() < 2e-4 * max(1.0, np.abs(want[:, 1:]).max()), tag
        if not use_edl:
            assert all(p['uncertainty'] == 0.0 for p in got)
        assert all(p['actionness'] == 0.0 for p in got)


@pytest.mark.parametrize("use_edl", [False, True])
def test_detect_batch_equals_the_per_video_path(use_edl):
    """detect_batch with a closed-set network (the head picks the decode, only the present keys are merged) against the
    reference's order of operations: per video prepare_clip -> net -> decode -> Soft-NMS -> duration clip."""
    from opental_amd.anet import test as A
    dev = torch.device("cuda", 0)
    net = closed_net(use_edl, seed=3).to(dev).eval()
    rs = np.random.RandomState(5)
    videos = [torch.from_numpy(rs.randint(0, 256, size=(3, t, 96, 96)).astype(np.uint8)).to(dev) for t in (768, 500)]
    fps, durations = [4.0, 5.0], [190.0, 99.0]
    got = A.detect_batch(net, videos, fps, durations, batch_clips=1)     # (a batch of 2 runs other conv kernels)
    from opental_amd.thumos14.test import softnms_classes
    total = 0
    for v, data in enumerate(videos):
        with torch.no_grad():
            out = net(A.prepare_clip(data, 0))
        dec = A.decode_clips(out, [fps[v]], os_head=False, use_edl=use_edl)
        rows, counts, _ = softnms_classes(dec, [0, 1], 5000, 0.85)
        ref = A.get_video_prediction(rows[0], counts[0], durations[v])
        assert got[v] == ref
        total += len(ref)
    assert total > 0


def _baseline_config(tmp_path, baseline, split_info=False):
    """tools/make_synthetic_anet.py's yaml rewritten to anet_softmax.yaml (focal loss, no os_head, no use_edl) or to
    anet_edl.yaml (edl_loss with its edl_config, use_edl, evidence exp, no os_head)."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    from make_synthetic_anet import make
    src = make(str(tmp_path / "data"), videos=4, size=100)
    cfg = yaml.load(open(src).read(), Loader=yaml.FullLoader)
    md, tr = cfg['model'], cfg['training']
    md.pop('os_head', None)
    if baseline == "softmax":
        md.pop('use_edl', None)
        tr['edl_loss'], tr['focal_loss'] = False, True
        tr.pop('edl_config', None)
    else:
        md['use_edl'], md['evidence'] = True, 'exp'
        tr['edl_loss'], tr['focal_loss'] = True, False
        tr['edl_config'] = dict(EDL_CFG)
    if split_info:                      # the test driver reads the validation subset, with fps and duration
        info = json.load(open(cfg['dataset']['training']['video_info_path']))
        for v in info.values():
            v.update(subset="validation", fps=10.0)
        path = str(tmp_path / "data" / "video_info_validation.json")
        json.dump(info, open(path, "w"))
        cfg['dataset']['testing']['video_info_path'] = path
        cfg['testing']['conf_thresh'] = 0.001       # anet/test.py filtering's default: random-init scores are ~1 / 302
    path = str(tmp_path / f"anet_{baseline}.yaml")
    with open(path, "w") as f:
        yaml.dump(cfg, f)
    return path


@pytest.fixture
def _restore_precision():
    from opental_amd.common import ops
    old = ops.CONV_PRECISION
    yield
    ops.CONV_PRECISION = old


@pytest.mark.parametrize("baseline", ["softmax", "edl"])
def test_lane_graph_steps_equal_eager_steps(tmp_path, baseline, _restore_precision):
    """A closed-set model and criterion from build_training: the capture's warm-up step plus three replayed lane-graph steps
    leave parameters and Adam moments BIT-IDENTICAL to four eager steps; the cost has no actionness terms."""
    import bench
    from opental_amd.anet.train import build_training
    from opental_amd.common import config as CF
    from opental_amd.common import ops
    dev = torch.device("cuda", 0)
    ops.CONV_PRECISION = 1
    cfg = CF.get_config([_baseline_config(tmp_path, baseline)] + BASE_FLAGS)
    clips, targets, scores = bench.synth_batch(2, 1000, dev, frames=768, classes=150, score_rows=3)

    def run(lanes):
        torch.manual_seed(7)
        net, crit, tr = build_training(cfg, dev, random_init=True)
        assert not net.os_head and crit.act_loss is None and net.num_classes == C
        assert crit.cls_loss_type == ('focal' if baseline == 'softmax' else 'edl')
        loc, conf, pri = torch.empty(2, 189, 2, device=dev), torch.empty(2, 189, C, device=dev), O.priors_all(arch.ANET).to(dev)
        assert crit._cls_mode(loc, conf, pri) == (3 if baseline == 'softmax' else 2)
        done = 0
        if lanes:
            tr.capture_step(clips, targets, scores, warmup=1, lanes=True)       # the warm-up step is a real step
            assert tr._graph[0] == "lanes"
            done = 1
        costs = []
        for _ in range(4 - done):
            r = tr.step(clips, targets, scores)
            if not lanes:
                assert r[1][-1] is None and r[1][-2] is None            # loss_act, loss_prop_act
            costs.append(float(r[0]))
        torch.cuda.synchronize()
        assert tr.step_count == 4
        return tr.arena.flat.detach().clone(), tr.arena.m.detach().clone(), costs, tr.replayed_steps
    pe, me, ce, _ = run(False)
    pl, ml, cl, replayed = run(True)
    assert replayed > 0 and all(np.isfinite(ce))
    assert torch.equal(pe, pl) and torch.equal(me, ml), float((pe - pl).abs().max())
    assert ce[-len(cl):] == cl, (ce, cl)


@pytest.mark.parametrize("baseline", ["softmax", "edl"])
def test_train_and_test_drivers_on_closed_set_configs(tmp_path, baseline, _restore_precision):
    """python -m opental_amd.anet.train / .test on the synthetic yaml rewritten to each baseline: two training steps, then
    the test driver writes a complete result file with the reference's fields (uncertainty 0.0 for Softmax, actionness
    0.0 for both)."""
    from opental_amd.anet import test as AT, train as AR
    path = _baseline_config(tmp_path, baseline, split_info=True)
    trainer, hist = AR.main([path] + BASE_FLAGS + ['--random_init', '--save_after', '0', '--max_steps', '2',
                                                   '--max_epoch', '1', '--checkpoint_path', str(tmp_path / "run")])
    assert not trainer.net.os_head and trainer.criterion.cls_loss_type == ('focal' if baseline == 'softmax' else 'edl')
    assert trainer.step_count == 2 and all(np.isfinite(h).all() for h in hist)
    ckpt = str(tmp_path / "run" / "checkpoint-1.ckpt")
    assert os.path.exists(ckpt)
    out_file = AT.main([path] + BASE_FLAGS[:3] + ['--checkpoint_path', ckpt])
    res = json.load(open(out_file))
    assert res['version'] == 'ActivityNet-v1.3' and sorted(res['results']) == [f'synth{i:05d}' for i in range(4)]
    props = [p for v in res['results'].values() for p in v]
    assert props
    for p in props[:500]:
        assert set(p) == {'label', 'score', 'segment', 'uncertainty', 'actionness'} and len(p['segment']) == 2
        assert p['actionness'] == 0.0 and (p['uncertainty'] == 0.0) == (baseline == 'softmax')
        assert p['label'].startswith('class_')
