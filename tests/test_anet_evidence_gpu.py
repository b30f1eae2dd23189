"""GPU: the EDL settings of the ActivityNet1.3 recipe beyond its shipped configs through otal_detection_loss_anet_ev
(detection_loss_anet_kernel<MODE, GEN = true>: the four lanes of an anchor share its row through csrc/evidence.h) -- against
tests/golden/anet_evidence.npz (tools/pin_anet_evidence.py), against the package's torch formulation at the shapes where the
quad layout can go wrong, at the decision edges against float64, the raw entry's contracts, and the captured training step."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import yaml

import anet_evidence_common as AE
import evidence_common as E

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUSED_NODE = 'AnetDetectionLossFunction'


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "anet_evidence.npz"))


def _fused(on):
    from opental_amd.anet import multisegment_loss as M
    M.FUSED = on


# ---- 1. the fixture
@pytest.mark.parametrize("name", list(AE.VARIANTS))
def test_fused_loss_matches_golden(fx, name):
    dev = torch.device("cuda", 0)
    os_head, _ = AE.VARIANTS[name]
    crit = AE.criterion(name, dev, epoch=int(fx["epoch"]))
    assert crit.fused_route()[0] == 'anet_ev'
    got = AE.call(crit, AE.head_outputs(int(fx["seed"]), os_head), AE.targets(fx), dev, weights=tuple(fx["weights"]))
    assert FUSED_NODE in got[2]
    AE.check_call(fx, name, got)


# ---- 2. against the torch formulation where the quad layout can go wrong
SHAPE_K = (3, 189, 257, 1024)       # less than one quad sweep, the recipe's value, one live quad in the second sweep, the limit
SHAPE_C = (2, 3, 5, 150)            # lanes that own no class; C mod 4 = 1, 2, 3
CASES = ("b1", "b1_none", "b2", "g1")
SHAPE_NAMES = ("relu_log", "softplus_digamma", "exp_mse", "closed_softplus_digamma_ibm")
# every K with every C; the sample layouts rotate over the grid, so that every K and every C meets all four of them
SHAPES = [(K, C, CASES[(i + j) % 4]) for i, K in enumerate(SHAPE_K) for j, C in enumerate(SHAPE_C)]


def synth_priors(K, dev):
    """(K, 2) priors for a K that is not the recipe's: centres (k + 0.5) / K, level ids k mod 6."""
    if K == 189:
        return AE.priors(dev)
    k = torch.arange(K, dtype=torch.float32)
    return torch.stack([(k + 0.5) / K, k % 6], 1).to(dev)


def synth_targets(case, K, labels, dev, seed):
    """Targets that are certain to give positives, whatever K: each is centred on an anchor of level 1..3 with max(left, right)
    in the middle of that level's bounds.  A sample without a positive gets one target outside the clip."""
    from opental_amd.anet.multisegment_loss import bounds
    rs = np.random.RandomState(seed)
    pri = synth_priors(K, "cpu").numpy()
    ok = [k for k in range(K) if 1 <= int(pri[k, 1]) <= 3 and 0.3 <= pri[k, 0] <= 0.7] or \
         [k for k in range(K) if 1 <= int(pri[k, 1]) <= 3]

    def row():
        k = ok[rs.randint(len(ok))]
        lo, hi = bounds[int(pri[k, 1])]
        h = 0.5 * (lo + hi) / 768.0
        return [float(pri[k, 0] - h), float(pri[k, 0] + h), float(rs.randint(1, labels + 1))]
    none = [[1.5, 1.6, 1.0]]
    per_sample = dict(b1=[[row(), row()]], b1_none=[none], b2=[[row(), row(), row()], none], g1=[[row()]])[case]
    return [torch.tensor(r, dtype=torch.float32, device=dev) for r in per_sample]


def synth_heads(seed, batch, K, C, os_head):
    """Head outputs for any K and C.  Every row of logits keeps a relu evidence sum e >= 1: the IoU calibration takes log(1 - u)
    with 1 - u = 1 - C / S = e / (C + e), whose float32 rounding error is 6e-8 (C + e) / e of its value -- at e = 0.005, C = 3
    (one row in four has no positive logit at all with C = 2, where u = 1 gives -inf, in the reference too) that is 4e-5 of the
    row's gradient, which float32 formulations of the same formula do differ by; with e >= 1 it stays below 4e-7 for C <= 5,
    and rows of 150 logits N(0, 2) carry e ~ 120.  A row below that gets 1 + |z| in its first logit."""
    rs = np.random.RandomState(seed)

    def logits():
        z = E.off_the_edges(rs.normal(0.0, 2.0, (batch, K, C)).astype(np.float32))
        weak = np.maximum(z, 0.0).sum(-1) < 1.0
        z[weak, 0] = 1.0 + np.abs(z[weak, 0])
        return z
    out = dict(loc=rs.uniform(4.0, 200.0, (batch, K, 2)).astype(np.float32),
               conf=logits(),
               prop_loc=rs.normal(0.0, 0.3, (batch, K, 2)).astype(np.float32),
               prop_conf=logits(),
               center=rs.normal(0.0, 1.0, (batch, K, 1)).astype(np.float32))
    if os_head:
        out["act"] = rs.normal(0.0, 1.0, (batch, K, 1)).astype(np.float32)
        out["prop_act"] = rs.normal(0.0, 1.0, (batch, K, 1)).astype(np.float32)
    return out


def _shape_criterion(name, C, dev):
    from opental_amd.anet.multisegment_loss import MultiSegmentLoss
    os_head, cfg = AE.VARIANTS[name]
    crit = MultiSegmentLoss(C, AE.PIOU, 1.0, cls_loss_type='edl', edl_config=dict(cfg), os_head=os_head).to(dev)
    crit.cls_loss.epoch = AE.EPOCH
    return crit


@pytest.mark.parametrize("K,C,case", SHAPES)
@pytest.mark.parametrize("name", SHAPE_NAMES)
def test_fused_loss_matches_torch_formulation(fx, name, K, C, case):
    """Fused against the torch formulation, both float32 on the device, two consecutive calls each."""
    dev = torch.device("cuda", 0)
    os_head = AE.VARIANTS[name][0]
    targets = synth_targets(case, K, C if os_head else C - 1, dev, seed=K + C)
    heads = synth_heads(1000 + K + C, len(targets), K, C, os_head)
    pri = synth_priors(K, dev)
    weights = (1.0, 0.7, 1.3, 0.9, 1.1, 0.8, 1.2)
    res = []
    for fused in (False, True):
        _fused(fused)
        try:
            crit = _shape_criterion(name, C, dev)
            calls = [AE.call(crit, heads, targets, dev, pri=pri, weights=weights) for _ in range(2)]
            assert all((FUSED_NODE in c[2]) == fused for c in calls)
            res.append(calls)
        finally:
            _fused(True)
    rt, rg = AE.tolerances(fx, name)
    for (l0, g0, _), (l1, g1, _) in zip(*res):
        print(name, K, C, case, l0.tolist(), l1.tolist())
        assert np.isfinite(l0).all() and np.isfinite(l1).all()
        assert (l0[0] > 0) == (case != "b1_none")               # the positives this case is meant to have
        assert np.allclose(l1, l0, rtol=rt, atol=1e-6), (l0, l1)
        for k in g0:
            scale = float(np.abs(g0[k]).max())
            err = float(np.abs(g0[k] - g1[k]).max())
            print(f"  grad {k}: max diff {err:.3e}, scale {scale:.3e}")
            assert err <= rg * max(scale, 1e-6), (k, err, scale)
    assert np.array_equal(res[1][0][0], res[1][1][0])           # no state: the second fused call repeats the first


# ---- 3. decision edges, against float64 autograd of the torch formulation on the same float32 inputs
def _edge_check(cfg, edit, os_head=True):
    dev = torch.device("cuda", 0)
    heads = AE.head_outputs(11, os_head, batch=1)
    for k in AE.GRAD_KEYS:
        edit(heads[k])
    tg = [AE.targets()[0]]
    got = AE.call(AE.criterion(cfg=cfg, os_head=os_head, dev=dev), heads, tg, dev)
    assert FUSED_NODE in got[2]
    want = AE.call(AE.criterion(cfg=cfg, os_head=os_head), heads, tg, "cpu", dtype=torch.float64)
    assert FUSED_NODE not in want[2]
    print(cfg, got[0].tolist(), want[0].tolist())
    assert np.isfinite(want[0]).all() and want[0][0] > 0
    np.testing.assert_allclose(got[0], want[0], rtol=2e-5, atol=1e-6)
    for k in got[1]:
        scale = float(np.abs(want[1][k]).max())
        err = float(np.abs(got[1][k] - want[1][k]).max())
        print(f"  grad {k}: max diff {err:.3e}, scale {scale:.3e}")
        assert err <= 2e-5 * max(scale, 1e-6), (k, err, scale)
    return got


@pytest.mark.parametrize("loss_type", E.LOSS_TYPES)
def test_relu_with_logits_of_exactly_zero(loss_type):
    def edit(z):
        z[:, ::2, 1::3] = 0.0
        z[:, 5::7, ::2] = -np.abs(z[:, 5::7, ::2])
        z[:, 5::7, 4] = 0.0
    _edge_check(dict(evidence='relu', loss_type=loss_type, iou_aware=True, **({} if loss_type == 'mse' else AE.IBM)), edit)


@pytest.mark.parametrize("loss_type", E.LOSS_TYPES)
def test_softplus_at_and_above_the_threshold(loss_type):
    def edit(z):
        z[:, ::2, 0] = 20.0
        z[:, 1::2, 3] = np.nextafter(np.float32(20.0), np.float32(np.inf))
        z[:, ::3, 7] = -30.0
        z[:, 2::5, 149] = 25.0
    _edge_check(dict(evidence='softplus', loss_type=loss_type, iou_aware=True, **({} if loss_type == 'mse' else AE.IBM)), edit)


@pytest.mark.parametrize("loss_type", ["digamma", "mse"])
def test_exp_at_the_clamp(loss_type):
    def edit(z):
        z[:, ::2, 0] = 10.0
        z[:, 1::2, 3] = -10.0
        z[:, ::3, 7] = np.nextafter(np.float32(10.0), np.float32(np.inf))
        z[:, 2::5, 148] = -12.0
    _edge_check(dict(evidence='exp', loss_type=loss_type, iou_aware=True, **({} if loss_type == 'mse' else AE.IBM)), edit)


@pytest.mark.parametrize("os_head,evidence,loss_type", [(True, 'softplus', 'digamma'), (True, 'exp', 'digamma'),
                                                        (False, 'exp', 'log'), (False, 'softplus', 'log')])
def test_rows_without_any_logit_under_ibm(os_head, evidence, loss_type):
    """|z|_1 = 0 in every third row: the weight is 1 / 1e-10, and sign(0) = 0 switches the gradient through |z|_1 off (abs'
    backward at 0).  iou_aware off: the calibration term of the untouched rows would vanish next to 1e10."""
    def edit(z):
        z[:, ::3] = 0.0
    got = _edge_check(dict(evidence=evidence, loss_type=loss_type, **AE.IBM), edit, os_head=os_head)
    assert got[0][1] > 1e9 and got[0][3] > 1e9


# ---- 4. the raw entry
def _raw_inputs(dev, os_head, B=2, K=189):
    C = AE.classes(os_head)
    h = AE.head_outputs(5, True, batch=B)
    if not os_head:
        h = dict(h, **{k: AE.head_outputs(5, False, batch=B)[k] for k in AE.GRAD_KEYS})
    for k in AE.GRAD_KEYS:                      # the decision edges of all three evidence functions among the logits
        h[k][:, ::4, 0], h[k][:, 1::4, 2], h[k][:, 2::4, 5], h[k][:, 3::4, 9] = 10.0, -10.0, 0.0, 20.0
        h[k][:, ::6, 11] = -12.0
    ins = {k: torch.from_numpy(v).to(dev).contiguous() for k, v in h.items()}
    ins["priors"] = AE.priors(dev).contiguous()
    ins["gt"] = torch.tensor([[[0.10, 0.30, 3.0], [0.45, 0.62, 77.0]], [[0.70, 0.95, 150.0], [0.05, 0.08, 12.0]]], device=dev)[:B].contiguous()
    ins["gvalid"] = torch.ones(B, 2, dtype=torch.uint8, device=dev)
    assert ins["conf"].shape == (B, K, C)
    return ins


def _raw(entry, mode, ins, ibm=0, kinds=None, expect=0, K=None):
    """One direct call of an ActivityNet detection-loss entry on device tensors: (losses, grads), pre-filled with NaN."""
    from opental_amd import _lib as L
    from opental_amd.anet.multisegment_loss import bounds
    lib = L.lib()
    B, Kt, C = ins["conf"].shape
    dev = ins["conf"].device
    losses = torch.full((7,), float('nan'), device=dev)
    grads = torch.full((lib.otal_detection_loss_grad_floats(B, Kt, C),), float('nan'), device=dev)
    scratch = torch.full((8 * B,), float('nan'), device=dev)
    closed = mode in (2, 3)
    p = lambda k: None if (closed and k in ("act", "prop_act")) else L.ptr(ins[k])
    lbs = (ctypes.c_float * 12)(*[float(v) for row in bounds for v in row])
    args = [p(k) for k in ("loc", "conf", "prop_loc", "prop_conf", "center", "act", "prop_act")] + [
        L.ptr(ins["priors"]), L.ptr(ins["gt"]), L.ptr(ins["gvalid"]), B, Kt if K is None else K, C, ins["gt"].shape[1], 768.0,
        0.6, lbs, 6, ibm, 10.0, 1, 0.1, 1.0, mode, 0.25]
    if kinds is not None:
        args += list(kinds)
    rc = getattr(lib, entry)(*args, L.ptr(losses), L.ptr(grads), L.ptr(scratch), L.stream())
    torch.cuda.synchronize()
    assert rc == expect, (entry, mode, rc)
    return losses, grads


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("mode,ibm", [(0, 0), (0, 1), (2, 0)])
def test_ev_entry_with_exp_log_is_the_ex_entry(mode, ibm):
    dev = torch.device("cuda", 0)
    ins = _raw_inputs(dev, mode == 0)
    old = _raw("otal_detection_loss_anet_ex", mode, ins, ibm=ibm)
    new = _raw("otal_detection_loss_anet_ev", mode, ins, ibm=ibm, kinds=(0, 0))
    assert _same_bits(old[0], new[0]) and _same_bits(old[1], new[1])
    assert float(old[0][1]) > 0 and bool(torch.isfinite(old[1]).all())


def test_refusals_write_nothing():
    dev = torch.device("cuda", 0)
    for mode in (0, 2):
        ins = _raw_inputs(dev, mode == 0)
        for kw in (dict(kinds=(1, 2), ibm=1), dict(kinds=(3, 0)), dict(kinds=(0, 3)), dict(kinds=(-1, 0)), dict(kinds=(2, 1), K=1025)):
            losses, grads = _raw("otal_detection_loss_anet_ev", mode, ins, expect=-7, **kw)
            assert bool(torch.isnan(losses).all()) and bool(torch.isnan(grads).all()), (mode, kw)
    losses, grads = _raw("otal_detection_loss_anet_ev", 3, _raw_inputs(dev, False), kinds=(1, 1), expect=-7)
    assert bool(torch.isnan(losses).all()) and bool(torch.isnan(grads).all())
    # otal_detection_loss_anet_ex keeps its refusal of IBM over the closed set
    _raw("otal_detection_loss_anet_ex", 2, _raw_inputs(dev, False), ibm=1, expect=-7)


@pytest.mark.parametrize("evidence,loss_type", [(0, 0)] + [(E.EVIDENCE.index(e), E.LOSS_TYPES.index(l)) for e, l in E.PAIRS])
def test_two_identical_launches_are_bitwise_identical(evidence, loss_type):
    """Modes 0 and 2 with IBM where the loss type takes it ((exp, log): the closed-set IBM instance only)."""
    dev = torch.device("cuda", 0)
    for mode in ((2,) if (evidence, loss_type) == (0, 0) else (0, 2)):
        ins = _raw_inputs(dev, mode == 0)
        ibm = int(loss_type != 2)
        first = _raw("otal_detection_loss_anet_ev", mode, ins, ibm=ibm, kinds=(evidence, loss_type))
        again = _raw("otal_detection_loss_anet_ev", mode, ins, ibm=ibm, kinds=(evidence, loss_type))
        assert _same_bits(first[0], again[0]) and _same_bits(first[1], again[1]), mode
        assert bool(torch.isfinite(first[0]).all()) and bool(torch.isfinite(first[1]).all())
        assert float(first[0][1]) > 0 and float(first[1].abs().max()) > 0


# ---- 5. the trainer
BASE_FLAGS = ['--open_set', '--split', '0', '--lw', '1', '--cw', '1', '--piou', '0.6']


def _sd_config(tmp_path):
    """tools/make_synthetic_anet.py's yaml rewritten to a closed-set (softplus, digamma) EDL config, as
    tests/test_anet_closed_set_gpu.py::_baseline_config builds anet_edl.yaml."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    from make_synthetic_anet import make
    src = make(str(tmp_path / "data"), videos=4, size=100)
    cfg = yaml.load(open(src).read(), Loader=yaml.FullLoader)
    md, tr = cfg['model'], cfg['training']
    md.pop('os_head', None)
    md['use_edl'], md['evidence'] = True, 'softplus'
    tr['edl_loss'], tr['focal_loss'] = True, False
    tr['edl_config'] = dict(evidence='softplus', loss_type='digamma')
    path = str(tmp_path / "anet_softplus_digamma.yaml")
    with open(path, "w") as f:
        yaml.dump(cfg, f)
    return path


def test_lane_graph_step_equals_eager_step_and_follows_the_kinds(tmp_path):
    """A (softplus, digamma) model and criterion from build_training: the capture's warm-up step plus one replayed lane-graph
    step leave parameters and Adam moments BIT-IDENTICAL to two eager steps; after the criterion's loss type changes, the next
    step is not a replay of that capture."""
    import bench
    from opental_amd.anet.train import build_training
    from opental_amd.common import config as CF
    from opental_amd.common import ops
    dev = torch.device("cuda", 0)
    old = ops.CONV_PRECISION
    ops.CONV_PRECISION = 1
    try:
        cfg = CF.get_config([_sd_config(tmp_path)] + BASE_FLAGS)
        clips, targets, scores = bench.synth_batch(2, 1000, dev, frames=768, classes=150, score_rows=3)

        def run(lanes):
            torch.manual_seed(7)
            net, crit, tr = build_training(cfg, dev, random_init=True)
            assert crit.fused_route() == ('anet_ev', 2, (2, 1), False)
            if lanes:
                tr.capture_step(clips, targets, scores, warmup=1, lanes=True)       # the warm-up step is a real step
                assert tr._graph[0] == "lanes"
            else:
                tr.step(clips, targets, scores)
            cost = float(tr.step(clips, targets, scores)[0])
            torch.cuda.synchronize()
            assert tr.step_count == 2
            return tr, crit, tr.arena.flat.detach().clone(), tr.arena.m.detach().clone(), cost
        _, _, pe, me, ce = run(False)
        tr, crit, pl, ml, cl = run(True)
        assert tr.replayed_steps == 1 and np.isfinite(ce)
        assert torch.equal(pe, pl) and torch.equal(me, ml), float((pe - pl).abs().max())
        assert ce == cl, (ce, cl)
        crit.cls_loss.loss_type = 'log'
        assert crit.fused_route() == ('anet_ev', 2, (2, 0), False) and tr._graph_key != tr._capture_key()
        tr.step(clips, targets, scores)
        torch.cuda.synchronize()
        assert tr.replayed_steps == 1 and tr.step_count == 3
    finally:
        ops.CONV_PRECISION = old
