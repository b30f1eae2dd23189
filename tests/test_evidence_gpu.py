"""GPU: the EDL settings beyond the final recipe (evidence relu / softplus, loss_type digamma / mse) through the single-launch loss
(csrc/loss.hip: otal_detection_loss_ev), the head tails (modes 3 / 4), the decode (otal_decode_clips_ev) and the anchor statistics
(otal_anchor_stats_ev) -- against tests/golden/evidence.npz (reference values, tools/pin_evidence.py), against the package's torch
formulation (float32 on the device, float64 on the host for the decision edges), the new entries against the existing ones bit
for bit, determinism, refusals, and the trainer and the drivers on a (softplus, digamma) configuration.

The head tails take the evidence kind as a mode number (2 exp, 3 relu, 4 softplus): exp through the new route IS mode 2."""
import os
import sys

import numpy as np
import pytest
import torch
import yaml

import ablations_common as A
import evidence_common as E

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WEIGHTS = dict(lw=1.0, cw=10.0, ctw=1.0, actw=1.0, ssl=0.001)
SENTINEL = -77.0


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "evidence.npz"))


def _targets(fx, dev):
    return [torch.from_numpy(fx["targets_0"]).to(dev), torch.from_numpy(fx["targets_1"]).to(dev)]


def _fused(on):
    from opental_amd.thumos14 import multisegment_loss as M
    M.FUSED = on


# ---- 4. the fused loss against the reference's values
@pytest.mark.parametrize("name", list(E.VARIANTS))
def test_fused_loss_matches_golden(fx, name):
    """Two consecutive calls at epoch 10 (the second reads the state the first left): terms, gradients, state."""
    dev = torch.device("cuda", 0)
    os_head, _ = E.VARIANTS[name]
    heads = E.head_outputs(int(fx["seed"]), 15 if os_head else 16, os_head)
    crit = E.criterion(name, dev, epoch=10)
    for tag in ("call1", "call2"):
        got = A.call(crit, heads, _targets(fx, dev), dev)
        assert 'DetectionLossFunction' in got[3], got[3]
        E.check_call(fx, name, tag, got)


# ---- 5. the fused loss against the torch formulation
def _case_targets(case, dev):
    """tests/test_ablations_gpu.py::_case_targets, rebuilt."""
    rs = np.random.RandomState(7)
    rows = lambda n: [[st, st + rs.uniform(0.05, 0.2), float(rs.randint(1, 16))] for st in rs.uniform(0.0, 0.8, n)]
    none = [[0.2505, 0.2575, 3.0]]              # no anchor centre inside: a sample without a positive
    per_sample = dict(b1=[rows(2)], b1_none=[none], b2=[rows(3), none])[case]
    return [torch.tensor(r, dtype=torch.float32, device=dev) for r in per_sample]


@pytest.mark.parametrize("name", E.OS_PAIRS)
@pytest.mark.parametrize("case", ["b1", "b1_none", "b2"])
def test_fused_loss_matches_torch_formulation(fx, name, case):
    """B = 1, B = 1 without any positive, B = 2 where one sample has none; two consecutive calls each."""
    dev = torch.device("cuda", 0)
    targets = _case_targets(case, dev)
    heads = E.head_outputs(100 + len(targets), 15, True, B=len(targets))
    res = []
    for fused in (False, True):
        _fused(fused)
        try:
            crit = E.criterion(name, dev, epoch=10)
            calls = [A.call(crit, heads, targets, dev) for _ in range(2)]
            assert all(('DetectionLossFunction' in c[3]) == fused for c in calls)
            res.append(calls)
        finally:
            _fused(True)
    rt, rg = E.tolerances(fx, name)
    for (l0, g0, s0, _), (l1, g1, s1, _) in zip(*res):
        print(name, case, l0.tolist(), l1.tolist())
        assert np.isfinite(l0).all() and np.isfinite(l1).all()
        assert np.allclose(l0, l1, rtol=rt, atol=1e-6), (l0, l1)
        for k in g0:
            scale = float(np.abs(g0[k]).max())
            assert float(np.abs(g0[k] - g1[k]).max()) <= rg * max(scale, 1e-6), (k, float(np.abs(g0[k] - g1[k]).max()), scale)


# ---- 6. decision edges, against float64 autograd of the torch formulation on the same float32 inputs
EDGE_TARGETS = [[[0.10, 0.30, 3.0], [0.45, 0.62, 7.0], [0.70, 0.95, 15.0]]]


def _edge_heads(edit):
    h = E.head_outputs(11, 15, True, B=1)
    for k in E.GRAD_KEYS:
        edit(h[k])
    return h


def _edge_check(cfg, heads):
    """One fused call on the device against the float64 torch formulation on the host: (fused terms, fused gradients)."""
    dev = torch.device("cuda", 0)
    tg = [torch.tensor(t, dtype=torch.float32) for t in EDGE_TARGETS]
    got = A.call(E.criterion(None, dev, cfg=cfg, os_head=True), heads, [t.to(dev) for t in tg], dev)
    assert 'DetectionLossFunction' in got[3]
    want = A.call(E.criterion(None, "cpu", cfg=cfg, os_head=True), {k: v.astype(np.float64) for k, v in heads.items()}, tg, "cpu")
    assert 'DetectionLossFunction' not in want[3]
    print(cfg['evidence'], cfg['loss_type'], got[0].tolist(), want[0].tolist())
    np.testing.assert_allclose(got[0], want[0], rtol=A.TOL, atol=1e-6)
    for k in got[1]:
        scale = float(np.abs(want[1][k]).max())
        err = float(np.abs(got[1][k] - want[1][k]).max())
        print(f"  grad {k}: max diff {err:.3e}, scale {scale:.3e}")
        assert err <= A.TOL * max(scale, 1e-6), (k, err, scale)
    return got[0], got[1]


@pytest.mark.parametrize("loss_type", ["log", "digamma"])
def test_relu_rows_without_evidence(loss_type):
    """Every logit <= 0 (negative values and exact zeros), iou_aware off: every counted row's term is log C (psi(C) - psi(1)
    for digamma), so both classification terms are that number, and the conf / prop_conf gradients are exactly 0."""
    def edit(z):
        z[...] = -np.abs(z)
        z[:, ::3, ::2] = 0.0
    cfg = dict(E.BASE, evidence='relu', loss_type=loss_type, iou_aware=False)
    terms, grads = _edge_check(cfg, _edge_heads(edit))
    want = float(np.log(15.0)) if loss_type == 'log' else float(torch.digamma(torch.tensor(15.0, dtype=torch.float64)) -
                                                                torch.digamma(torch.tensor(1.0, dtype=torch.float64)))
    np.testing.assert_allclose(terms[[1, 3]], want, rtol=A.TOL)
    assert not grads["conf"].any() and not grads["prop_conf"].any()


@pytest.mark.parametrize("loss_type", E.LOSS_TYPES)
def test_relu_with_logits_of_exactly_zero(loss_type):
    def edit(z):
        z[:, ::2, 1::3] = 0.0
        z[:, 5::7] = -np.abs(z[:, 5::7])            # and some counted rows with no evidence at all
        z[:, 5::7, 4] = 0.0
    _edge_check(dict(E.BASE, evidence='relu', loss_type=loss_type, iou_aware=False), _edge_heads(edit))


@pytest.mark.parametrize("loss_type", E.LOSS_TYPES)
def test_softplus_at_and_above_the_threshold(loss_type):
    def edit(z):
        z[:, ::2, 0] = 20.0
        z[:, 1::2, 3] = np.nextafter(np.float32(20.0), np.float32(np.inf))
        z[:, ::3, 7] = -30.0
        z[:, 2::5, 9] = 25.0
    _edge_check(dict(E.BASE, evidence='softplus', loss_type=loss_type), _edge_heads(edit))


@pytest.mark.parametrize("loss_type", ["digamma", "mse"])
def test_exp_at_the_clamp_through_the_new_entry(loss_type):
    def edit(z):
        z[:, ::2, 0] = 10.0
        z[:, 1::2, 3] = -10.0
        z[:, ::3, 7] = np.nextafter(np.float32(10.0), np.float32(np.inf))
        z[:, 2::5, 9] = -12.0
    _edge_check(dict(E.BASE, evidence='exp', loss_type=loss_type), _edge_heads(edit))


# ---- 7 - 9. the raw entries
def _raw(entry, mode, ins, reweight=None, ibm=0, bins=50, momentum=0.99, kinds=None, expect=0):
    """One direct call of a detection-loss entry on device tensors: (losses, grads, state), pre-filled with a sentinel."""
    from opental_amd import _lib as L
    lib = L.lib()
    B, K, C = ins["conf"].shape
    dev = ins["conf"].device
    losses = torch.full((7,), SENTINEL, device=dev)
    grads = torch.full((lib.otal_detection_loss_grad_floats(B, K, C),), SENTINEL, device=dev)
    scratch = torch.zeros(lib.otal_detection_loss_scratch_floats(B, K), device=dev)
    state = torch.linspace(0.5, 1.5, bins, device=dev)
    closed = mode in (2, 3)
    p = lambda k: None if (closed and k in ("act", "prop_act")) else L.ptr(ins[k])
    args = [p(k) for k in ("loc", "conf", "prop_loc", "prop_conf", "center", "act", "prop_act")] + [
        L.ptr(ins["priors"]), L.ptr(ins["gt"]), L.ptr(ins["gvalid"]), L.ptr(state), B, K, C, 1, 256.0, 0.5, ibm, bins,
        momentum, 1, mode, 0.25]
    if reweight is not None:
        args += [reweight, 2.0]
    if kinds is not None:
        args += list(kinds)
    rc = getattr(lib, entry)(*args, L.ptr(losses), L.ptr(grads), L.ptr(scratch), L.stream())
    torch.cuda.synchronize()
    assert rc == expect, (entry, mode, rc)
    return losses, grads, state


def _raw_inputs(dev, B=2):
    h = E.head_outputs(5, 16, True, B=B)
    for k in E.GRAD_KEYS:                       # the decision edges of all three evidence functions among the logits
        h[k][:, ::4, 0], h[k][:, 1::4, 2], h[k][:, 2::4, 5], h[k][:, 3::4, 9] = 10.0, -10.0, 0.0, 20.0
        h[k][:, ::6, 11] = -12.0
    ins = {k: torch.from_numpy(v).to(dev).contiguous() for k, v in h.items()}
    ins["priors"] = A.priors(dev)[:, 0].contiguous()
    ins["gt"] = torch.tensor([[[0.10, 0.30, 3.0]], [[0.45, 0.62, 7.0]]], device=dev)[:B].contiguous()
    ins["gvalid"] = torch.ones(B, 1, dtype=torch.uint8, device=dev)
    return ins


RAW_RULES = [(0, 0, 0), (0, 1, 0), (0, 2, 0), (0, 3, 0), (0, 0, 1), (2, 0, 0), (2, 1, 0), (2, 2, 0), (2, 3, 0), (2, 0, 1)]


@pytest.mark.parametrize("mode,reweight,ibm", RAW_RULES)
def test_ev_entry_with_exp_log_is_the_ex_entry(mode, reweight, ibm):
    dev = torch.device("cuda", 0)
    ins = _raw_inputs(dev)
    old = _raw("otal_detection_loss_ex", mode, ins, reweight=reweight, ibm=ibm, bins=30, momentum=0.85)
    new = _raw("otal_detection_loss_ev", mode, ins, reweight=reweight, ibm=ibm, bins=30, momentum=0.85, kinds=(0, 0))
    for a, b in zip(old, new):
        assert torch.equal(a, b)
    assert float(old[0][1]) > 0 and bool(torch.isfinite(old[1]).all())


@pytest.mark.parametrize("evidence,loss_type", [(E.EVIDENCE.index(e), E.LOSS_TYPES.index(l)) for e, l in E.PAIRS])
def test_two_identical_calls_are_bitwise_identical(evidence, loss_type):
    dev = torch.device("cuda", 0)
    ins = _raw_inputs(dev)
    rules = RAW_RULES if loss_type != 2 else [(0, 0, 0), (2, 0, 0)]
    for mode, reweight, ibm in rules:
        first = _raw("otal_detection_loss_ev", mode, ins, reweight=reweight, ibm=ibm, bins=30, momentum=0.85,
                     kinds=(evidence, loss_type))
        again = _raw("otal_detection_loss_ev", mode, ins, reweight=reweight, ibm=ibm, bins=30, momentum=0.85,
                     kinds=(evidence, loss_type))
        for a, b in zip(first, again):
            assert torch.equal(a, b) and bool(torch.isfinite(a).all()), (mode, reweight, ibm)
        assert float(first[0][1]) > 0 and float(first[1].abs().max()) > 0
        if reweight == 2 or ibm:
            assert not torch.equal(first[2], torch.linspace(0.5, 1.5, 30, device=dev))


def test_refusals_write_nothing():
    dev = torch.device("cuda", 0)
    ins = _raw_inputs(dev)
    fresh = torch.linspace(0.5, 1.5, 30, device=dev)
    bad = [dict(kinds=(1, 2), ibm=1), dict(kinds=(2, 2), reweight=1), dict(kinds=(0, 2), reweight=2), dict(kinds=(1, 2), reweight=3),
           dict(kinds=(3, 0)), dict(kinds=(-1, 0)), dict(kinds=(0, 3)), dict(kinds=(0, -1))]
    for kw in bad:
        for mode in (0, 2):
            kw = dict(dict(reweight=0, ibm=0), **kw)
            losses, grads, state = _raw("otal_detection_loss_ev", mode, ins, bins=30, momentum=0.85, expect=-7, **kw)
            assert bool((losses == SENTINEL).all()) and bool((grads == SENTINEL).all()) and torch.equal(state, fresh), kw
    _raw("otal_detection_loss_ev", 1, ins, reweight=0, kinds=(1, 1), expect=-7)


def test_decode_ev_with_exp_is_the_ex_entry(fx):
    from opental_amd.common import detect as D
    dev = torch.device("cuda", 0)
    for os_head in (True, False):
        out = _decode_inputs(fx, os_head, dev)
        old = D.decode_clips(out, [c[0] for c in E.CLIPS], [c[1] for c in E.CLIPS], 256, E.CONF_THRESH, os_head=os_head)
        calls = []
        from opental_amd import _lib as L
        check = L.check
        L.check = lambda rc, what: (calls.append(what), check(rc, what))[1]
        try:
            ev = D.EVIDENCE
            D.EVIDENCE = dict(ev, exp_again=0)          # the same kind under a name that takes the _ev route
            new = D.decode_clips(out, [c[0] for c in E.CLIPS], [c[1] for c in E.CLIPS], 256, E.CONF_THRESH, os_head=os_head,
                                 evidence='exp_again')
        finally:
            L.check, D.EVIDENCE = check, ev
        assert calls == ["otal_decode_clips_ev"]
        for k in ("seg", "score", "unct", "flag") + (("actn",) if os_head else ()):
            assert torch.equal(old[k], new[k]), k


# ---- 10. head tails
@pytest.mark.parametrize("kind", ["relu", "softplus"])
@pytest.mark.parametrize("shape", [(2, 15, 126), (1, 150, 189)])
def test_head_tails_uncertainty_forward_and_backward(kind, shape):
    """The Dirichlet item of the head-tail launch for relu / softplus against float64 autograd of compute_uncertainty; the
    logits hold 0 and 20 exactly."""
    from opental_amd.common import ops
    from opental_amd.thumos14.BDNet import DirichletLayer
    dev = torch.device("cuda", 0)
    B, C, N = shape
    rs = np.random.RandomState(B * 1000 + C)
    raw = rs.normal(0.0, 3.0, shape).astype(np.float32)
    raw[:, ::3, ::5], raw[:, 1::4, 2::7], raw[:, 2, 3] = 0.0, 20.0, 25.0
    w_out, w_u = rs.normal(0.0, 1.0, (B, N, C)).astype(np.float32), rs.normal(0.0, 1.0, (B, N)).astype(np.float32)
    x = torch.from_numpy(raw).to(dev).requires_grad_(True)
    scale = torch.ones(1, device=dev)
    out, unct = ops.HeadOutputsFunction.apply((0, N), None, (ops.HEAD_UNCT_MODE[kind],), scale, x)
    ((out * torch.from_numpy(w_out).to(dev)).sum() + (unct * torch.from_numpy(w_u).to(dev)).sum()).backward()
    x64 = torch.from_numpy(raw).double().requires_grad_(True)
    o64 = x64.permute(0, 2, 1)
    u64 = DirichletLayer(kind).compute_uncertainty(o64)
    ((o64 * torch.from_numpy(w_out).double()).sum() + (u64 * torch.from_numpy(w_u).double()).sum()).backward()
    assert torch.equal(out.detach().cpu(), torch.from_numpy(raw).permute(0, 2, 1))
    np.testing.assert_allclose(unct.detach().cpu().numpy(), u64.detach().numpy(), rtol=1e-6, atol=0)
    g, want = x.grad.cpu().numpy(), x64.grad.numpy()
    err, top = float(np.abs(g - want).max()), float(np.abs(want).max())
    print(f"{kind} {shape}: max grad diff {err:.3e}, scale {top:.3e}")
    assert err <= 2e-5 * top


def test_bdnet_asks_for_the_matching_head_item():
    from opental_amd.anet import BDNet as anet
    from opental_amd.common import ops
    from opental_amd.thumos14.BDNet import BDNet, DEFAULT_MODEL_CFG
    for kind in E.EVIDENCE:
        net = BDNet(in_channels=3, training=False, use_edl=True, cfg=dict(DEFAULT_MODEL_CFG, evidence=kind))
        assert net.coarse_pyramid_detection.dirichlet_mode == ops.HEAD_UNCT_MODE[kind] == 2 + E.EVIDENCE.index(kind)
    assert BDNet(in_channels=3, training=False, use_edl=False).coarse_pyramid_detection.dirichlet_mode == 0
    for kind in E.EVIDENCE:         # the ActivityNet recipe, through the shared CoarsePyramid
        net = anet.BDNet(in_channels=3, training=False, use_edl=True, cfg=dict(anet.DEFAULT_MODEL_CFG, evidence=kind))
        assert net.coarse_pyramid_detection.dirichlet_mode == ops.HEAD_UNCT_MODE[kind]


# ---- 11. decode
def _decode_inputs(fx, os_head, dev):
    h = E.head_outputs(int(fx["seed"]), 15 if os_head else 16, os_head)
    out = {k: torch.from_numpy(v).to(dev) for k, v in h.items()}
    out["priors"] = A.priors(dev)
    return out


@pytest.mark.parametrize("os_head", [True, False])
@pytest.mark.parametrize("kind", ["relu", "softplus"])
def test_decode_matches_reference(fx, kind, os_head):
    """otal_decode_clips_ev against the reference's decode_predictions: segments (1e-6 / 1e-5, the comparison of
    tests/test_infer_gpu.py) and flags exact; scores, uncertainty and actionness rtol 1e-5 (atol 1e-7), as there."""
    from opental_amd.common.detect import decode_clips
    dev = torch.device("cuda", 0)
    dec = decode_clips(_decode_inputs(fx, os_head, dev), [c[0] for c in E.CLIPS], [c[1] for c in E.CLIPS], 256, E.CONF_THRESH,
                       os_head=os_head, use_edl=True, evidence=kind)
    tag = f"dec_{kind}_{'os' if os_head else 'closed'}"
    for ci in range(2):
        np.testing.assert_allclose(dec["seg"][ci].cpu().numpy(), fx[f"{tag}_seg_{ci}"], rtol=1e-6, atol=1e-5)
        np.testing.assert_allclose(dec["score"][ci].cpu().numpy(), fx[f"{tag}_score_{ci}"], rtol=1e-5, atol=1e-7)
        np.testing.assert_allclose(dec["unct"][ci].cpu().numpy(), fx[f"{tag}_unct_{ci}"], rtol=1e-5, atol=1e-7)
        if os_head:
            np.testing.assert_allclose(dec["actn"][ci].cpu().numpy(), fx[f"{tag}_actn_{ci}"], rtol=1e-5, atol=1e-7)
        assert np.array_equal(dec["flag"][ci].cpu().numpy(), fx[f"{tag}_mask_{ci}"])
        assert fx[f"{tag}_mask_{ci}"].any() and not fx[f"{tag}_mask_{ci}"].all()
    assert dec["actn"] is not None if os_head else dec["actn"] is None


# ---- 12. anchor statistics
def _stats_case(kind):
    """The THUMOS14 launch of tests/anchor_stats_cases.py (B = 2, K = 126, C = 15, G = 4; sample 1 without a positive) with the
    rows that miss a bin margin UNDER THIS EVIDENCE drawn again, so that a float32 rounding cannot move an anchor to another
    bin."""
    import copy
    from anchor_stats_cases import BINS, MARGIN, _draw_rows, _frac, case, reference, targets_of
    c = copy.deepcopy(case('thumos_no_positive'))
    rs = np.random.RandomState(5)
    for _ in range(200):
        bad = np.zeros(c['loc'].shape[:2], bool)
        for t in targets_of(c):
            r = reference(c, t, evidence=kind)
            ds = _frac(r['value'].astype(np.float64) * BINS, BINS, False)
            dg = np.where(r['counts'], _frac(np.abs(r['grad']).astype(np.float64) * BINS, BINS, False), np.inf)
            bad |= (ds < MARGIN).any(-1) | (dg < MARGIN).any(-1)
        bad |= (np.abs(r['iou'].astype(np.float64) - c['overlap_thresh']) < MARGIN)
        if not bad.any():
            return c
        _draw_rows(rs, c, bad)
    raise AssertionError("no margin-safe case")


@pytest.mark.parametrize("target", ['uncertainty', 'confidence', 'half_au'])
@pytest.mark.parametrize("kind", ["relu", "softplus"])
def test_anchor_stats_ev_matches_the_host_rule(kind, target):
    """Labels and both histograms exactly; values rtol 1e-5 / atol 1e-7, gradients 2e-5 of the largest |g| (the comparison of
    tests/test_anchor_stats_gpu.py, whose recorded spread of 1.0e-7 is below the 2e-5 floor)."""
    from anchor_stats_cases import BINS, INPUTS, reference
    from opental_amd.common import ops
    c = _stats_case(kind)
    want = reference(c, target, evidence=kind)
    ins = [None if c[k] is None else torch.from_numpy(c[k]).cuda() for k in INPUTS]
    res = ops.anchor_stats(*ins, c['clip_length'], c['overlap_thresh'], c['os_head'], c['n_known'], target, BINS, BINS, evidence=kind)
    got = {k: v.cpu().numpy() for k, v in res.items()}
    exp = reference(c, target)
    assert not np.array_equal(want['hist_grad'], exp['hist_grad']) and not np.allclose(want['value'], exp['value'])   # not exp's
    assert np.array_equal(got['label'], want['label'])
    assert np.array_equal(got['hist_score'], want['hist_score']) and np.array_equal(got['hist_grad'], want['hist_grad'])
    np.testing.assert_allclose(got['value'], want['value'], rtol=1e-5, atol=1e-7)
    gmax = max(float(np.abs(want['grad']).max()), 1e-30)
    assert np.abs(got['grad'] - want['grad']).max() <= 2e-5 * gmax
    assert (got['grad'][~want['counts']] == 0.0).all() and want['counts'].any()


def test_anchor_stats_ev_with_exp_is_the_existing_entry():
    from anchor_stats_cases import BINS, CLIP, INPUTS, OVERLAP, case
    from opental_amd import _lib as L
    from opental_amd.common import ops
    c = case('thumos_no_positive')
    ins = [None if c[k] is None else torch.from_numpy(c[k]).cuda() for k in INPUTS]
    old = ops.anchor_stats(*ins, CLIP, OVERLAP, True, 15, 'half_au', BINS, BINS)
    B, K, C = c['conf'].shape
    new = dict(hist_score=torch.zeros_like(old['hist_score']), hist_grad=torch.zeros_like(old['hist_grad']),
               label=torch.zeros_like(old['label']), value=torch.zeros_like(old['value']), grad=torch.zeros_like(old['grad']))
    rc = L.lib().otal_anchor_stats_ev(*[L.ptr(t) for t in ins], B, K, C, c['gt'].shape[1], CLIP,
                                      OVERLAP, 1, 15, 4, BINS, BINS,
                                      *[L.ptr(new[k]) for k in ('hist_score', 'hist_grad', 'label', 'value', 'grad')], 0, L.stream())
    torch.cuda.synchronize()
    assert rc == 0
    for k in new:
        assert torch.equal(old[k], new[k]), k


# ---- 13. the trainer
def _net(evidence, seed=5):
    from opental_amd.thumos14.BDNet import BDNet, DEFAULT_MODEL_CFG
    torch.manual_seed(seed)
    net = BDNet(in_channels=3, training=False, use_edl=True, cfg=dict(DEFAULT_MODEL_CFG, os_head=True, evidence=evidence))
    net.backbone._model.apply(BDNet.weight_init)
    return net


def test_lane_graph_steps_equal_eager_steps():
    """(softplus, digamma) with IBM, os_head, b = 2: five steps under lane-graph capture leave parameters, Adam moments and the
    IBM state BIT-IDENTICAL to five eager steps."""
    import bench
    from opental_amd.common import ops
    from opental_amd.thumos14.train import DetectorTrainer
    dev = torch.device("cuda", 0)
    old = ops.CONV_PRECISION
    ops.CONV_PRECISION = 1
    try:
        clips, targets, scores = bench.synth_batch(2, 1000, dev)

        def run(lanes):
            crit = E.criterion("sd_ibm", dev, epoch=10)
            tr = DetectorTrainer(_net('softplus').to(dev).train(), crit, WEIGHTS, lr=1e-4, weight_decay=1e-3)
            fresh = crit.cls_loss.state().clone()
            if lanes:
                tr.capture_step(clips, targets, scores, warmup=1, lanes=True)       # the warm-up step is a real step
                assert tr._graph[0] == "lanes"
            else:
                tr.step(clips, targets, scores)
            costs = [float(tr.step(clips, targets, scores)[0]) for _ in range(4)]
            torch.cuda.synchronize()
            assert tr.step_count == 5 and not torch.equal(crit.cls_loss.state(), fresh)
            assert crit._cls_mode(clips[:, :, 0, 0, :2]) == 0 and crit._kinds() == (2, 1)
            return tr.arena.flat.detach().clone(), tr.arena.m.detach().clone(), costs, tr.replayed_steps, crit.cls_loss.state().clone()
        pe, me, ce, _, se = run(False)
        pl, ml, cl, replayed, sl = run(True)
        assert replayed >= 3 and all(np.isfinite(ce))
        assert torch.equal(pe, pl) and torch.equal(me, ml), float((pe - pl).abs().max())
        assert torch.equal(se, sl) and ce == cl, (ce, cl)
    finally:
        ops.CONV_PRECISION = old


# ---- 14. the drivers
def test_train_then_detect_on_a_softplus_digamma_config(tmp_path, monkeypatch):
    """Two steps of thumos14.train.main on the synthetic set with model.evidence softplus and edl_config (softplus, digamma):
    the criterion's launches are otal_detection_loss_ev.  Then the detection pipeline on one video with that network: finite
    rows whose uncertainty column is C / sum(softplus(z) + 1), averaged over the two stages, of the raw maps."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    from make_synthetic_thumos import make
    from opental_amd import _lib as L
    from opental_amd.common import detect as D
    from opental_amd.common import ops
    from opental_amd.thumos14 import test as T
    from opental_amd.thumos14 import train as R
    precision = ops.CONV_PRECISION
    src = make(str(tmp_path / "data"), videos=2, frames=400, size=100)
    cfg = yaml.load(open(src).read(), Loader=yaml.FullLoader)
    cfg['model']['os_head'], cfg['model']['use_edl'], cfg['model']['evidence'] = True, True, 'softplus'
    cfg['training']['edl_loss'], cfg['training']['focal_loss'] = True, False
    cfg['training']['edl_config'] = dict(E.SD, **dict(E.IBM, ibm_start=1))
    cfg['training']['act_config'] = dict(A.ACT)
    path = str(tmp_path / "softplus_digamma.yaml")
    with open(path, "w") as f:
        yaml.dump(cfg, f)
    launches = []
    check = L.check
    monkeypatch.setattr(L, 'check', lambda rc, what: (launches.append(what), check(rc, what))[1])
    flags = ['--open_set', '--split', '0', '--lw', '1', '--cw', '10', '--piou', '0.5', '--ssl', '0.001', '--batch_size', '2',
             '--random_init', '--save_after', '0', '--max_epoch', '1', '--checkpoint_path', str(tmp_path / "run"), '--max_steps', '2']
    try:
        trainer, hist = R.main([path] + flags)
        cl = trainer.criterion.cls_loss
        assert trainer.net.evidence == 'softplus' and (cl.evidence, cl.loss_type, cl.reweight()) == ('softplus', 'digamma', 'ibm')
        assert trainer.step_count == 2 and all(np.isfinite(h).all() for h in hist)
        assert launches.count("otal_detection_loss_ev") >= 1 and "otal_detection_loss" not in launches \
            and "otal_detection_loss_ex" not in launches
        assert not torch.equal(cl.state().cpu(), torch.ones(50))
        net = trainer.net.eval()
        assert D.head_mode(net) == (True, True, 'softplus') and net.coarse_pyramid_detection.dirichlet_mode == 4
        data_path = cfg['dataset']['training']['video_data_path']
        name = sorted(n[:-4] for n in os.listdir(data_path) if n.endswith('.npy'))[0]
        video = D.prepare_data(data_path, name, 96, 'cuda')
        seen = []
        forward_windows = D.forward_windows
        monkeypatch.setattr(D, 'forward_windows', lambda *a, **k: (seen.append(forward_windows(*a, **k)), seen[-1])[1])
        del launches[:]
        rows, counts, index, dec = T.detect_batch(net, [video], [10.0], conf_thresh=1e-4)
        torch.cuda.synchronize()
    finally:
        ops.CONV_PRECISION = precision
    assert "otal_decode_clips_ev" in launches and "otal_decode_clips" not in launches
    C = 15
    u = lambda z: C / (torch.nn.functional.softplus(z.double()) + 1).sum(-1)
    want = ((u(seen[0]['conf']) + u(seen[0]['prop_conf'])) / 2.0).cpu().numpy()
    np.testing.assert_allclose(dec['unct'].cpu().numpy(), want, rtol=1e-5, atol=1e-7)
    rows, counts, index = rows[0].cpu().numpy(), counts[0].cpu().numpy(), index[0].cpu().numpy()
    assert int(counts.sum()) > 0 and rows.shape[-1] == 5
    flat = want.reshape(-1)
    for k in range(rows.shape[0]):
        r = rows[k, :counts[k]]
        assert np.isfinite(r).all()
        np.testing.assert_allclose(r[:, 3], flat[index[k, :counts[k]]], rtol=1e-5, atol=1e-7)
