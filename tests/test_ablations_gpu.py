"""GPU: the THUMOS14 loss ablations through the single-launch loss (csrc/loss.hip: otal_detection_loss_ex) -- against
tests/golden/ablations.npz (reference values), against the package's torch formulation, the extended entry against the existing
one bit for bit, run-to-run determinism, and the training driver on a ghm and on the noACT config (lane graphs across the
start epoch, checkpoint round trip of the loss state)."""
import os
import sys

import numpy as np
import pytest
import torch
import yaml

import ablations_common as A

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WEIGHTS = dict(lw=1.0, cw=10.0, ctw=1.0, actw=1.0, ssl=0.001)


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "ablations.npz"))


def _targets(fx, dev):
    return [torch.from_numpy(fx["targets_0"]).to(dev), torch.from_numpy(fx["targets_1"]).to(dev)]


def _fused(on):
    from opental_amd.thumos14 import multisegment_loss as M
    M.FUSED = on


@pytest.mark.parametrize("name", list(A.VARIANTS))
def test_fused_loss_matches_golden(fx, name):
    """Both calls at epoch 10 (the second one reads the state the first one left) and the call at epoch 0: terms, gradients
    and the state vector against the reference's."""
    dev = torch.device("cuda", 0)
    os_head, _ = A.VARIANTS[name]
    heads = A.head_outputs(int(fx["seed"]), 15 if os_head else 16, os_head)
    crit = A.criterion(name, dev, epoch=10)
    for tag in ("call1", "call2"):
        got = A.call(crit, heads, _targets(fx, dev), dev)
        assert 'DetectionLossFunction' in got[3], got[3]
        A.check_call(fx, name, tag, got, A.grads_tag(fx, name, tag))
    got = A.call(A.criterion(name, dev, epoch=0), heads, _targets(fx, dev), dev)
    assert 'DetectionLossFunction' in got[3]
    A.check_call(fx, name, "epoch0", got)


def _case_targets(case, dev):
    rs = np.random.RandomState(7)
    rows = lambda n: [[st, st + rs.uniform(0.05, 0.2), float(rs.randint(1, 16))] for st in rs.uniform(0.0, 0.8, n)]
    none = [[0.2505, 0.2575, 3.0]]              # no anchor centre inside: a sample without a positive
    per_sample = dict(b1=[rows(2)], b1_none=[none], b2=[rows(3), none])[case]
    return [torch.tensor(r, dtype=torch.float32, device=dev) for r in per_sample]


@pytest.mark.parametrize("name", list(A.VARIANTS))
@pytest.mark.parametrize("case", ["b1", "b1_none", "b2"])
def test_fused_loss_matches_torch_formulation(fx, name, case):
    """B = 1, B = 1 without any positive (M = 0 in both passes: GHM must update nothing), B = 2 with one such sample; two
    consecutive calls each, so the state the kernel leaves is what the torch formulation leaves."""
    dev = torch.device("cuda", 0)
    os_head, _ = A.VARIANTS[name]
    targets = _case_targets(case, dev)
    heads = A.head_outputs(100 + len(targets), 15 if os_head else 16, os_head, B=len(targets))
    res = []
    for fused in (False, True):
        _fused(fused)
        try:
            crit = A.criterion(name, dev, epoch=10)
            calls = [A.call(crit, heads, targets, dev) for _ in range(2)]
            assert all(('DetectionLossFunction' in c[3]) == fused for c in calls)
            res.append(calls)
        finally:
            _fused(True)
    rt, rg = A.tolerances(fx, name)
    for (l0, g0, s0, _), (l1, g1, s1, _) in zip(*res):
        assert np.allclose(l0, l1, rtol=rt, atol=1e-6), (l0, l1)
        np.testing.assert_allclose(s1, s0, rtol=A.TOL, atol=1e-7)
        for k in g0:
            scale = float(np.abs(g0[k]).max())
            assert float(np.abs(g0[k] - g1[k]).max()) <= rg * max(scale, 1e-6), (k, float(np.abs(g0[k] - g1[k]).max()), scale)
    if case == "b1_none" and name in ("ghm", "hardmib", "noIoUC"):
        fresh = A.state_of(A.criterion(name, dev))
        assert np.array_equal(res[1][1][2], fresh)         # no row counted: the state is untouched


def _raw(entry, mode, ins, reweight=None, ibm=0, bins=50, momentum=0.99):
    """One direct call of otal_detection_loss / otal_detection_loss_ex on device tensors: (losses, grads, state)."""
    from opental_amd import _lib as L
    lib = L.lib()
    B, K, C = ins["conf"].shape
    dev = ins["conf"].device
    losses = torch.zeros(7, device=dev)
    grads = torch.zeros(lib.otal_detection_loss_grad_floats(B, K, C), device=dev)
    scratch = torch.zeros(lib.otal_detection_loss_scratch_floats(B, K), device=dev)
    state = torch.linspace(0.5, 1.5, bins, device=dev)
    closed = mode in (2, 3)
    p = lambda k: None if (closed and k in ("act", "prop_act")) else L.ptr(ins[k])
    args = [p(k) for k in ("loc", "conf", "prop_loc", "prop_conf", "center", "act", "prop_act")] + [
        L.ptr(ins["priors"]), L.ptr(ins["gt"]), L.ptr(ins["gvalid"]), L.ptr(state), B, K, C, 1, 256.0, 0.5, ibm, bins,
        momentum, 1, mode, 0.25]
    if reweight is not None:
        args += [reweight, 2.0]
    rc = getattr(lib, entry)(*args, L.ptr(losses), L.ptr(grads), L.ptr(scratch), L.stream())
    torch.cuda.synchronize()
    assert rc == 0, (entry, mode, rc)
    return losses, grads, state


def _raw_inputs(dev, B=2):
    h = A.head_outputs(5, 16, True, B=B)
    ins = {k: torch.from_numpy(v).to(dev).contiguous() for k, v in h.items()}
    ins["priors"] = A.priors(dev)[:, 0].contiguous()
    ins["gt"] = torch.tensor([[[0.10, 0.30, 3.0]], [[0.45, 0.62, 7.0]]], device=dev)[:B].contiguous()
    ins["gvalid"] = torch.ones(B, 1, dtype=torch.uint8, device=dev)
    return ins


@pytest.mark.parametrize("mode,ibm", [(0, 0), (0, 1), (1, 0), (2, 0), (3, 0)])
def test_ex_entry_with_reweight_0_is_the_existing_entry(mode, ibm):
    dev = torch.device("cuda", 0)
    ins = _raw_inputs(dev)
    old = _raw("otal_detection_loss", mode, ins, ibm=ibm)
    new = _raw("otal_detection_loss_ex", mode, ins, reweight=0, ibm=ibm)
    for a, b in zip(old, new):
        assert torch.equal(a, b)


@pytest.mark.parametrize("mode,reweight,ibm", [(0, 1, 0), (0, 2, 0), (0, 3, 0), (2, 1, 0), (2, 2, 0), (2, 3, 0), (2, 0, 1)])
def test_two_identical_calls_are_bitwise_identical(mode, reweight, ibm):
    dev = torch.device("cuda", 0)
    ins = _raw_inputs(dev)
    first = _raw("otal_detection_loss_ex", mode, ins, reweight=reweight, ibm=ibm, bins=30, momentum=0.85)
    again = _raw("otal_detection_loss_ex", mode, ins, reweight=reweight, ibm=ibm, bins=30, momentum=0.85)
    for a, b in zip(first, again):
        assert torch.equal(a, b) and bool(torch.isfinite(a).all())
    assert float(first[0][1]) > 0 and float(first[1].abs().max()) > 0
    if reweight == 2 or ibm:
        assert not torch.equal(first[2], torch.linspace(0.5, 1.5, 30, device=dev))        # the state moved


def _net(os_head, seed=5):
    from opental_amd.thumos14.BDNet import BDNet, DEFAULT_MODEL_CFG
    torch.manual_seed(seed)
    net = BDNet(in_channels=3, training=False, use_edl=True, cfg=dict(DEFAULT_MODEL_CFG, os_head=os_head))
    net.backbone._model.apply(BDNet.weight_init)
    return net


@pytest.mark.parametrize("name", ["ghm", "noACT"])
def test_lane_graph_steps_equal_eager_steps_across_the_start_epoch(name):
    """Two steps at epoch 9 (rule inactive) and three at epoch 10 (active): the captured run -- whose key changes with the
    epoch, so it steps eagerly once and captures again -- leaves parameters, Adam moments and the loss state BIT-IDENTICAL to
    five eager steps."""
    import bench
    from opental_amd.common import ops
    from opental_amd.thumos14.train import DetectorTrainer
    dev = torch.device("cuda", 0)
    old = ops.CONV_PRECISION
    ops.CONV_PRECISION = 1
    try:
        clips, targets, scores = bench.synth_batch(2, 1000, dev)

        def run(lanes):
            crit = A.criterion(name, dev, epoch=9)
            tr = DetectorTrainer(_net(A.VARIANTS[name][0]).to(dev).train(), crit, WEIGHTS, lr=1e-4, weight_decay=1e-3)
            fresh = crit.cls_loss.state().clone()
            if lanes:
                tr.capture_step(clips, targets, scores, warmup=1, lanes=True)       # the warm-up step is a real step
                assert tr._graph[0] == "lanes"
            else:
                tr.step(clips, targets, scores)
            tr.step(clips, targets, scores)
            assert torch.equal(crit.cls_loss.state(), fresh)                         # below the start epoch: no update
            crit.cls_loss.epoch = 10
            costs = [float(tr.step(clips, targets, scores)[0]) for _ in range(3)]
            torch.cuda.synchronize()
            assert tr.step_count == 5 and not torch.equal(crit.cls_loss.state(), fresh)
            return tr.arena.flat.detach().clone(), tr.arena.m.detach().clone(), costs, tr.replayed_steps, crit.cls_loss.state().clone()
        pe, me, ce, _, se = run(False)
        pl, ml, cl, replayed, sl = run(True)
        assert replayed >= 3 and all(np.isfinite(ce))
        assert torch.equal(pe, pl) and torch.equal(me, ml), float((pe - pl).abs().max())
        assert torch.equal(se, sl) and ce == cl, (ce, cl)
    finally:
        ops.CONV_PRECISION = old


@pytest.fixture
def _restore_precision():
    from opental_amd.common import ops
    old = ops.CONV_PRECISION
    yield
    ops.CONV_PRECISION = old


@pytest.mark.parametrize("name", ["ghm", "noACT"])
def test_train_driver_and_resume_on_ablation_configs(tmp_path, name, _restore_precision):
    """The synthetic yaml with this ablation's model.os_head and training.edl_config (start epoch 1, so that the two steps
    of epoch 1 run the rule): two training steps, then a resumed run reads the loss state back from the checkpoint."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    from make_synthetic_thumos import make
    from opental_amd.thumos14 import train as R
    src = make(str(tmp_path / "data"), videos=2, frames=400, size=100)
    cfg = yaml.load(open(src).read(), Loader=yaml.FullLoader)
    os_head, edl = A.VARIANTS[name]
    cfg['model']['os_head'] = os_head
    cfg['model']['use_edl'], cfg['model']['evidence'] = True, 'exp'
    cfg['training']['edl_loss'], cfg['training']['focal_loss'] = True, False
    cfg['training']['edl_config'] = dict(edl, **({'ghm_start': 1} if name == "ghm" else {'ibm_start': 1}))
    cfg['training']['act_config'] = dict(A.ACT)
    path = str(tmp_path / f"{name}.yaml")
    with open(path, "w") as f:
        yaml.dump(cfg, f)
    flags = ['--open_set', '--split', '0', '--lw', '1', '--cw', '10', '--piou', '0.5', '--ssl', '0.001', '--batch_size', '2',
             '--random_init', '--save_after', '0', '--max_epoch', '1', '--checkpoint_path', str(tmp_path / "run")]
    trainer, hist = R.main([path] + flags + ['--max_steps', '2'])
    cl = trainer.criterion.cls_loss
    assert trainer.net.os_head == os_head and cl.reweight() == ('ghm' if name == "ghm" else 'ibm')
    assert trainer.step_count == 2 and all(np.isfinite(h).all() for h in hist)
    state = cl.state().detach().clone()
    fresh = torch.zeros(30) if name == "ghm" else torch.ones(50)
    assert trainer._ibm_state() is cl.state() and not torch.equal(state.cpu(), fresh)
    resumed, hist2 = R.main([path] + flags + ['--resume', '1'])
    assert not hist2 and resumed is not trainer
    assert torch.equal(resumed.criterion.cls_loss.state().cpu(), state.cpu())
    key = 'acc_sum' if name == "ghm" else 'weight_accum'
    st = torch.load(str(tmp_path / "run" / "training" / "checkpoint_1.ckpt"), map_location='cpu', weights_only=False)
    assert torch.equal(st[key], state.cpu())
