"""CPU: the EDL settings beyond the final recipe (evidence relu / softplus, loss_type digamma / mse) -- opental_amd/csrc/evidence.h
through a g++ harness against torch float64, the package's torch formulation against tests/golden/evidence.npz (written from the
reference by tools/pin_evidence.py), and the new entries of the library (declared, exported, argument checks; no launch)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ablations_common as A
import evidence_common as E

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("otal_detection_loss_ev", "otal_decode_clips_ev", "otal_anchor_stats_ev")


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "evidence.npz"))


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    return E.build_harness(tmp_path_factory.mktemp("cpu_evidence"))


@pytest.fixture(scope="module")
def lib():
    from opental_amd.csrc import build
    if not os.path.exists(build.LIB):
        build.build(verbose=False)
    from opental_amd._lib import declare
    return declare(ctypes.CDLL(build.LIB))


def _ulp(x, up):
    return np.nextafter(np.float32(x), np.float32(np.inf if up else -np.inf))


# ---- 1. evidence.h against float64
def test_alpha_and_dalpha_on_the_edges(H):
    """alpha and d alpha / d z of the three evidence functions on a grid with every decision edge and its float neighbours,
    against torch float64 autograd of the package's _evidence on the same float32 inputs (torch's backward conventions: clamp
    inclusive, relu 0 at 0, softplus 1 above the threshold)."""
    grid = np.array([-30.0, -10.0, _ulp(-10, False), _ulp(-10, True), 0.0, _ulp(0, False), _ulp(0, True), 10.0, _ulp(10, False),
                     _ulp(10, True), 20.0, _ulp(20, True), 25.0, -3.7, 0.5, 4.0, 15.0, 19.5], np.float32)
    for ev, kind in enumerate(E.EVIDENCE):
        z = torch.from_numpy(grid).double().requires_grad_(True)
        a = E.torch_evidence(z, kind) + 1
        a.sum().backward()
        got_a, got_d = E.harness_map(H, "cpu_ev_alpha", grid, ev), E.harness_map(H, "cpu_ev_dalpha", grid, ev)
        np.testing.assert_allclose(got_a, a.detach().numpy(), rtol=2e-7, atol=0, err_msg=kind)
        np.testing.assert_allclose(got_d, z.grad.numpy(), rtol=3e-7, atol=1e-12, err_msg=kind)
    # the conventions, literally
    d = lambda ev, v: float(E.harness_map(H, "cpu_ev_dalpha", np.array([v], np.float32), ev)[0])
    assert d(0, 10.0) > 2e4 and d(0, -10.0) > 0 and d(0, _ulp(10, True)) == 0.0 and d(0, _ulp(-10, False)) == 0.0
    assert d(1, 0.0) == 0.0 and d(1, _ulp(0, True)) == 1.0 and d(1, _ulp(0, False)) == 0.0
    assert d(2, _ulp(20, True)) == 1.0 and 0.0 < d(2, 4.0) < 1.0 and 0.0 < d(2, -30.0) < 1e-12       # (sigmoid(20) rounds to 1.0f)


def test_digamma_and_trigamma_against_float64(H):
    """~2000 log-spaced points of [1, 4e5], 1.0 itself and the neighbourhood of digamma's zero.  Error = |got - f64| / max(1,
    |f64|); bound = 4 x the largest error torch's own float32 digamma / polygamma(1, .) make on the same grid (the project's
    margin over a reference's own float32 error), no less than 1e-6."""
    x = np.concatenate([np.exp(np.linspace(0.0, np.log(4e5), 2000)), [1.0], np.linspace(1.4516, 1.4716, 41),
                        [1.4616321449683623]]).astype(np.float32)
    x64 = torch.from_numpy(x).double()
    for name, fn in (("cpu_ev_digamma", torch.digamma), ("cpu_ev_trigamma", lambda t: torch.polygamma(1, t))):
        ref = fn(x64).numpy()
        err = lambda got: float((np.abs(got.astype(np.float64) - ref) / np.maximum(1.0, np.abs(ref))).max())
        mine, torch32 = err(E.harness_map(H, name, x)), err(fn(torch.from_numpy(x)).numpy())
        bound = max(1e-6, 4.0 * torch32)
        print(f"{name}: largest error {mine:.3e}; torch float32 {torch32:.3e}; bound {bound:.3e}")
        assert mine <= bound, f"{name}: largest error {mine:.3e}, torch float32 {torch32:.3e}, bound {bound:.3e}"
    # relative accuracy where the gradient needs it: psi'(S) is ~1 / S at S ~ 3.5e5
    big = x > 2.0
    got = E.harness_map(H, "cpu_ev_trigamma", x)[big].astype(np.float64)
    ref = torch.polygamma(1, x64).numpy()[big]
    assert float((np.abs(got - ref) / ref).max()) <= 1e-6


@pytest.mark.parametrize("lt", range(3))
@pytest.mark.parametrize("ev", range(3))
def test_row_term_and_its_derivative_against_float64(H, ev, lt):
    """cls_row / cls_dalpha on 64 rows of 15 logits (some rows all <= 0, some past the clamp and the softplus threshold)
    against float64 autograd of the reference's formulas with respect to alpha."""
    rs = np.random.RandomState(3)
    z = rs.normal(0.0, 3.0, (64, 15)).astype(np.float32)
    z[0] = -np.abs(z[0])
    z[1, 3], z[2, 5], z[3, :4] = 24.0, 11.0, (-12.0, 20.0, 0.0, 10.0)
    y = rs.randint(0, 15, 64).astype(np.int32)
    per, d = E.harness_rows(H, z, y, ev, lt)
    al = (E.torch_evidence(torch.from_numpy(z).double(), E.EVIDENCE[ev]) + 1).requires_grad_(True)
    S = al.sum(1, keepdim=True)
    yy = torch.from_numpy(y).long()
    if lt == 2:
        oh = F.one_hot(yy, 15).double()
        want = ((oh - al / S) ** 2).sum(1) + (al * (S - al) / (S * S * (S + 1))).sum(1)
    else:
        f = torch.log if lt == 0 else torch.digamma
        want = (f(S) - f(al.gather(1, yy[:, None]))).view(-1)
    want.sum().backward()
    np.testing.assert_allclose(per, want.detach().numpy(), rtol=2e-6, atol=2e-6)
    g = al.grad.numpy()
    scale = np.abs(g).max(1, keepdims=True)
    assert float((np.abs(d - g) / scale).max()) <= 2e-6


# ---- 2. the torch formulation against the fixture
def _targets(fx):
    return [torch.from_numpy(fx["targets_0"]), torch.from_numpy(fx["targets_1"])]


@pytest.mark.parametrize("name", list(E.VARIANTS))
def test_host_formulation_matches_reference(fx, name):
    os_head, _ = E.VARIANTS[name]
    heads = E.head_outputs(int(fx["seed"]), 15 if os_head else 16, os_head)
    crit = E.criterion(name, epoch=10)
    for tag in ("call1", "call2"):
        got = A.call(crit, heads, _targets(fx))
        assert 'DetectionLossFunction' not in got[3]
        E.check_call(fx, name, tag, got)


def test_fixture_is_what_the_issue_asks_for(fx, golden_dir):
    assert os.path.getsize(os.path.join(golden_dir, "evidence.npz")) <= os.path.getsize(os.path.join(golden_dir, "ablations.npz"))
    for name in E.VARIANTS:
        for tag in ("call1", "call2"):
            assert np.isfinite(fx[f"{name}_{tag}_terms"]).all()
        assert (f"{name}_call2_grad_conf" in fx.files) == (name in E.STATEFUL)
    for os_head in (True, False):
        h = E.head_outputs(int(fx["seed"]), 15 if os_head else 16, os_head)
        for k in E.GRAD_KEYS:
            assert min(float(np.abs(h[k] - e).min()) for e in E.EDGES) >= E.EDGE_MARGIN
    # relu with iou_aware: no counted row of the refined stage has all logits <= 0
    assert not (E.head_outputs(int(fx["seed"]), 15, True)["prop_conf"] <= 0).all(-1).any()


@pytest.mark.parametrize("kind", ["relu", "softplus"])
def test_dirichlet_layer_uncertainty_matches_reference(fx, kind):
    from opental_amd.thumos14.BDNet import DirichletLayer
    heads = E.head_outputs(int(fx["seed"]), 15, True)
    layer = DirichletLayer(kind)
    for k in E.GRAD_KEYS:
        np.testing.assert_allclose(layer.compute_uncertainty(torch.from_numpy(heads[k])).numpy(), fx[f"unct_{kind}_{k}"],
                                   rtol=1e-6, atol=0)


def test_cls_mode_covers_the_nine_pairs_and_refuses_mse_with_a_rule():
    """_cls_mode needs a device tensor to say yes; its refusal does not: 'mse' with a re-weighting rule or IBM configured is
    never the kernel's, whatever the tensor."""
    class Dev:                      # what _cls_mode reads of `loc`
        is_cuda, dtype, shape = True, torch.float32, (2, 126, 2)
    for e in E.EVIDENCE:
        for l in E.LOSS_TYPES:
            for os_head in (True, False):
                crit = E.criterion(None, cfg=dict(E.BASE, evidence=e, loss_type=l), os_head=os_head)
                assert crit._cls_mode(Dev) == (0 if os_head else 2), (e, l, os_head)
                assert crit._kinds() == (E.EVIDENCE.index(e), E.LOSS_TYPES.index(l))
    for rule in (dict(E.IBM), dict(with_focal=True), dict(with_ghm=True, num_bins=30, momentum=0.85), dict(with_ibloss=True)):
        crit = E.criterion(None, cfg=dict(E.BASE, evidence='relu', loss_type='mse', **rule), os_head=True)
        assert crit._cls_mode(Dev) is None, rule
        assert E.criterion(None, cfg=dict(E.BASE, evidence='relu', loss_type='digamma', **rule), os_head=True)._cls_mode(Dev) == 0


def _thumos_criterion(kind, os_head, cfg=None, epoch=10, **kw):
    from opental_amd.thumos14.multisegment_loss import MultiSegmentLoss
    key = dict(edl='edl_config', rpl='rpl_config').get(kind)
    crit = MultiSegmentLoss(15 if os_head else 16, 0.5, 1.0, cls_loss_type=kind, os_head=os_head,
                            act_config=kw.pop('act_config', dict(A.ACT)), **({key: dict(cfg)} if key else {}), **kw)
    if kind == 'edl':
        crit.cls_loss.epoch = epoch
    return crit


FINAL = dict(A.BASE, **A.IBM)           # thumos14_opental_final.yaml
PLAIN0 = ('plain', 0, None, 0, False)
SD = (2, 1)                             # (softplus, digamma) as csrc/evidence.h numbers them
# (how the criterion is built) -> fused_route(), written out from the branches the dispatch had inside DetectionLossFunction.forward
# (_ev when the pair is not (exp, log), else _ex with a rule in force or IBM active over a closed set, else the plain entry) and
# inside MultiSegmentLoss.forward / _cls_mode (the mode, the rule of EvidenceLoss.reweight() at the epoch)
THUMOS_ROUTES = [
    (lambda: _thumos_criterion('edl', True, FINAL, 9), PLAIN0),
    (lambda: _thumos_criterion('edl', True, FINAL, 10), ('plain', 0, None, 0, True)),
    # the eight ablation variants on both sides of their start epoch (10 in every yaml; focal is ungated)
    (lambda: A.criterion("focal", epoch=9), ('ex', 0, None, 1, False)),
    (lambda: A.criterion("focal", epoch=10), ('ex', 0, None, 1, False)),
    (lambda: A.criterion("ghm", epoch=9), PLAIN0),
    (lambda: A.criterion("ghm", epoch=10), ('ex', 0, None, 2, False)),
    (lambda: A.criterion("ghm0", epoch=9), PLAIN0),
    (lambda: A.criterion("ghm0", epoch=10), ('ex', 0, None, 2, False)),
    (lambda: A.criterion("ib", epoch=9), PLAIN0),
    (lambda: A.criterion("ib", epoch=10), ('ex', 0, None, 3, False)),
    (lambda: A.criterion("hardmib", epoch=9), PLAIN0),
    (lambda: A.criterion("hardmib", epoch=10), ('plain', 0, None, 0, True)),
    (lambda: A.criterion("noMIB", epoch=9), PLAIN0),
    (lambda: A.criterion("noMIB", epoch=10), PLAIN0),
    (lambda: A.criterion("noIoUC", epoch=9), PLAIN0),
    (lambda: A.criterion("noIoUC", epoch=10), ('plain', 0, None, 0, True)),
    (lambda: A.criterion("noACT", epoch=9), ('plain', 2, None, 0, False)),
    (lambda: A.criterion("noACT", epoch=10), ('ex', 2, None, 0, True)),
    # the eight pairs other than (exp, log), and the other variants of the evidence fixture
    (lambda: E.criterion("exp_digamma"), ('ev', 0, (0, 1), 0, False)),
    (lambda: E.criterion("exp_mse"), ('ev', 0, (0, 2), 0, False)),
    (lambda: E.criterion("relu_log"), ('ev', 0, (1, 0), 0, False)),
    (lambda: E.criterion("relu_digamma"), ('ev', 0, (1, 1), 0, False)),
    (lambda: E.criterion("relu_mse"), ('ev', 0, (1, 2), 0, False)),
    (lambda: E.criterion("softplus_log"), ('ev', 0, (2, 0), 0, False)),
    (lambda: E.criterion("softplus_digamma"), ('ev', 0, SD, 0, False)),
    (lambda: E.criterion("softplus_mse"), ('ev', 0, (2, 2), 0, False)),
    (lambda: E.criterion("closed_relu_log"), ('ev', 2, (1, 0), 0, False)),
    (lambda: E.criterion("closed_softplus_digamma"), ('ev', 2, SD, 0, False)),
    (lambda: E.criterion("closed_exp_mse"), ('ev', 2, (0, 2), 0, False)),
    (lambda: E.criterion("sd_ibm", epoch=9), ('ev', 0, SD, 0, False)),
    (lambda: E.criterion("sd_ibm", epoch=10), ('ev', 0, SD, 0, True)),
    (lambda: E.criterion("sd_focal"), ('ev', 0, SD, 1, False)),
    (lambda: E.criterion("sd_ghm", epoch=9), ('ev', 0, SD, 0, False)),
    (lambda: E.criterion("sd_ghm", epoch=10), ('ev', 0, SD, 2, False)),
    (lambda: E.criterion("sd_ib", epoch=10), ('ev', 0, SD, 3, False)),
    (lambda: _thumos_criterion('edl', False, dict(E.SD, **E.IBM), 10), ('ev', 2, SD, 0, True)),
    # mse with a rule or IBM configured: the torch formulation, before the start epoch too
    (lambda: _thumos_criterion('edl', True, dict(E.BASE, evidence='relu', loss_type='mse', **E.IBM), 3), None),
    (lambda: _thumos_criterion('edl', False, dict(E.BASE, evidence='exp', loss_type='mse', **E.IBM), 10), None),
    (lambda: _thumos_criterion('edl', True, dict(E.BASE, evidence='relu', loss_type='mse', with_focal=True), 10), None),
    (lambda: _thumos_criterion('edl', True, dict(E.BASE, evidence='relu', loss_type='mse', with_ghm=True, num_bins=30, momentum=0.85), 10), None),
    (lambda: _thumos_criterion('edl', True, dict(E.BASE, evidence='softplus', loss_type='mse', with_ibloss=True), 10), None),
    (lambda: _thumos_criterion('edl', True, dict(FINAL, num_bins=65), 10), None),          # more bins than the kernel's 64
    # focal (the as-shipped dispatch and thumos14_softmax.yaml), RPL / GCPL
    (lambda: _thumos_criterion('focal', True), ('plain', 1, None, 0, False)),
    (lambda: _thumos_criterion('focal', False), ('plain', 3, None, 0, False)),
    (lambda: _thumos_criterion('rpl', False, dict(temperature=1, weight_pl=0.1)), ('rpl', 'rpl', None, 0, False)),
    (lambda: _thumos_criterion('rpl', False, dict(temperature=1, weight_pl=0.1, gcpl=True)), ('rpl', 'rpl', None, 0, False)),
    (lambda: _thumos_criterion('rpl', False, dict(temperature=0, weight_pl=0.1)), None),
    (lambda: _thumos_criterion('rpl', False, dict(temperature=-1, weight_pl=0.1, gcpl=True)), None),
    # size_average, and an actionness rank term with a weight: the torch formulation
    (lambda: _thumos_criterion('edl', True, FINAL, 10, size_average=True), None),
    (lambda: _thumos_criterion('focal', False, size_average=True), None),
    (lambda: _thumos_criterion('edl', True, FINAL, 10, act_config=dict(margin=1.0, weight=0.1)), None),
    (lambda: _thumos_criterion('focal', True, act_config=dict(margin=1.0, weight=0.1)), None),
]


@pytest.mark.parametrize("make, want", THUMOS_ROUTES, ids=[f"{i:02d}-" + ("torch" if w is None else f"{w[0]}-mode{w[1]}-rw{w[3]}" + "-ibm" * w[4])
                                                           for i, (_, w) in enumerate(THUMOS_ROUTES)])
def test_thumos_fused_route_table(make, want):
    """fused_route() reads the criterion's settings and its epoch only; _cls_mode is that route's mode behind the tensor gate."""
    from opental_amd.thumos14 import multisegment_loss as M
    crit = make()
    assert crit.fused_route() == want

    class Dev:                      # what the tensor gate reads of `loc`
        is_cuda, dtype, shape = True, torch.float32, (2, 126, 2)
    class Big(Dev):                 # one anchor past the kernel's 2048
        shape = (1, 2049, 2)
    assert crit._cls_mode(Dev) == (None if want is None else want[1]) and crit._fused_ok(Dev) == (want is not None)
    assert crit._cls_mode(Big) is None and crit._cls_mode(torch.zeros(2, 126, 2)) is None
    assert crit._cls_mode(torch.zeros(2, 126, 2, dtype=torch.float64)) is None
    M.FUSED = False
    try:
        assert crit.fused_route() is None and crit._cls_mode(Dev) is None      # FUSED = False forces the torch formulation
    finally:
        M.FUSED = True


def test_a_focal_alpha_that_is_not_the_kernels_form_keeps_the_torch_formulation():
    """The kernels take FocalLoss_Ori(balance_index 0, gamma 2): alpha for class 0 and 1 - alpha for every other class."""
    from opental_amd.thumos14.cls_loss import FocalLoss_Ori
    from opental_amd.thumos14.multisegment_loss import kernel_focal_alpha0
    assert kernel_focal_alpha0(FocalLoss_Ori(16, balance_index=0, size_average=False, alpha=0.25)) == 0.25
    others = (FocalLoss_Ori(16, balance_index=3, size_average=False, alpha=0.25),             # alpha[0] + alpha[1] = 1.5
              FocalLoss_Ori(16, balance_index=0, size_average=False, alpha=0.25, gamma=3),
              FocalLoss_Ori(16, size_average=False, alpha=[0.25] + [0.75] * 14 + [0.5]))      # not one alpha for the others
    for os_head in (True, False):
        crit = _thumos_criterion('focal', os_head)
        assert crit._focal_alpha0 == 0.25 and crit.fused_route() is not None
        for focal in others:
            crit.cls_loss, crit._focal_alpha0 = focal, kernel_focal_alpha0(focal)
            assert crit._focal_alpha0 is None and crit.fused_route() is None


def test_capture_key_holds_the_pair():
    from opental_amd.thumos14.train import DetectorTrainer
    import inspect
    src = inspect.getsource(DetectorTrainer._capture_key)
    assert "'evidence'" in src and "'loss_type'" in src


# ---- 3. symbols
def test_new_entries_are_declared_and_exported(lib):
    txt = open(os.path.join(REPO, "include", "opental_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in NEW_ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
        assert hasattr(lib, name), name
    assert lib.otal_abi_version() == 26


def test_argument_checks_of_the_new_entries(lib):
    """Refusals come before any read or launch: the pointers here are never dereferenced."""
    one = ctypes.c_void_p(16)
    unsupported = -7

    def loss(evidence, loss_type, cls_mode=0, ibm=0, reweight=0, act=one):
        return lib.otal_detection_loss_ev(one, one, one, one, one, act, act, one, one, one, one, 1, 126, 15, 1, 256.0, 0.5,
                                          ibm, 50, 0.99, 1, cls_mode, 0.25, reweight, 2.0, evidence, loss_type, one, one,
                                          one, None)
    for bad in ((3, 0), (-1, 0), (0, 3), (0, -1)):
        assert loss(*bad) == unsupported, bad
    assert loss(1, 2, ibm=1) == unsupported                     # mse with IBM
    for rw in (1, 2, 3):
        assert loss(2, 2, reweight=rw) == unsupported           # mse with a re-weighting rule
    assert loss(1, 1, cls_mode=1) == unsupported and loss(1, 1, cls_mode=3) == unsupported      # the focal modes take no evidence
    assert loss(1, 1, act=None) == -1                           # the OpenTAL mode needs the actionness maps

    def decode(evidence, score_fn=0):
        return lib.otal_decode_clips_ev(one, one, one, one, one, one, one, one, one, one, one, one, one, one, one, 1, 126, 15,
                                        256.0, 0.01, score_fn, 0, evidence, None)
    assert decode(3) == unsupported and decode(-1) == unsupported and decode(1, score_fn=2) == unsupported

    def stats(evidence):
        return lib.otal_anchor_stats_ev(one, one, one, one, one, one, one, one, one, 1, 126, 15, 1, 256.0, 0.5, 1, 15, 0, 100,
                                        100, one, one, None, None, None, evidence, None)
    assert stats(3) == unsupported and stats(-1) == unsupported
    modes = (ctypes.c_int * 1)(5)
    chans = (ctypes.c_int * 1)(15)
    lev = (ctypes.c_int * 2)(0, 126)
    ptrs = (ctypes.c_void_p * 1)(16)
    assert lib.otal_head_outputs_fwd(1, chans, modes, ptrs, ptrs, ptrs, None, 1, 126, 1, lev, None, None) == -2     # mode 5


def test_decode_refuses_an_unknown_evidence_name():
    from opental_amd.common.detect import decode_clips
    with pytest.raises(NotImplementedError):
        decode_clips({'loc': torch.zeros(1, 126, 2), 'conf': torch.zeros(1, 126, 15)}, [0.0], [10.0], evidence='tanh')


@pytest.mark.parametrize("kind", ["relu", "softplus"])
@pytest.mark.parametrize("os_head", [True, False])
def test_decode_ev_refuses_host_tensors(kind, os_head):
    """otal_decode_clips_ev reads device memory: host tensors are refused before any pointer is taken."""
    from opental_amd.common.detect import decode_clips
    z = lambda *s: torch.zeros(*s)
    out = dict(loc=z(1, 126, 2), prop_loc=z(1, 126, 2), conf=z(1, 126, 15), prop_conf=z(1, 126, 15), center=z(1, 126, 1),
               act=z(1, 126, 1), prop_act=z(1, 126, 1), priors=z(126, 1))
    with pytest.raises(NotImplementedError, match="device tensors only"):
        decode_clips(out, [0.0], [10.0], os_head=os_head, use_edl=True, evidence=kind)
