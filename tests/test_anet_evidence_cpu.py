"""CPU: the EDL settings of the ActivityNet1.3 recipe beyond its shipped configs (evidence relu / softplus, loss_type digamma /
mse, IBM over the closed set) -- the lane-share row functions of opental_amd/csrc/evidence.h through a g++ harness against
torch float64 and against the serial cls_row, the package's torch formulation against tests/golden/anet_evidence.npz (written
from the reference by tools/pin_anet_evidence.py), the routing of the criterion's settings to the library's entries, and
otal_detection_loss_anet_ev (declared, exported, argument checks; no launch)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import anet_evidence_common as AE
import evidence_common as E

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROW_C = (2, 3, 5, 150, 151)


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "anet_evidence.npz"))


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    return AE.build_harness(tmp_path_factory.mktemp("cpu_evidence_lanes"))


@pytest.fixture(scope="module")
def lib():
    from opental_amd.csrc import build
    if not os.path.exists(build.LIB):
        build.build(verbose=False)
    from opental_amd._lib import declare
    return declare(ctypes.CDLL(build.LIB))


# ---- 1. the lane-share rows against float64 and against cls_row
def _rows(C):
    """32 rows of C logits (one all <= 0, some past the clamp and the softplus threshold, the decision edges themselves) and
    labels: class 0 (the first lane's share), the last class of the last lane that owns one, C - 1, and -1 (not classified).
    The logit past the clamp (24: alpha = e^10 + 1) sits in a class that is NOT its row's label: with it in the labelled class of a 2- or 3-class row p_y = 1 - 5e-5 and the mse derivative is
    what is left of a cancellation -- torch's own float32 autograd of the reference's formula misses float64 by 1.8e-5 (C = 2)
    and 3.2e-5 (C = 3) of the row's largest element there, so that row measures the number format, not these functions."""
    rs = np.random.RandomState(100 + C)
    z = rs.normal(0.0, 3.0, (32, C)).astype(np.float32)
    z[0] = -np.abs(z[0])
    last_of_lane3 = max((c for c in range(C) if c % 4 == 3), default=C - 1)
    y = np.array([(0, last_of_lane3, C - 1, -1)[i % 4] for i in range(32)], np.int32)
    z[1, (y[1] + 1) % C], z[2, 0] = 24.0, 11.0
    z[3, :2] = (-12.0, 20.0)
    z[4, :2] = (0.0, 10.0)
    return z, y


def _float64_rows(z, y, ev, lt):
    """(per, d per / d alpha) in float64 for the classified rows (y >= 0), by autograd of the reference's formulas."""
    C = z.shape[1]
    al = (E.torch_evidence(torch.from_numpy(z).double(), E.EVIDENCE[ev]) + 1).requires_grad_(True)
    S = al.sum(1, keepdim=True)
    yy = torch.from_numpy(y).long().clamp(min=0)
    if lt == 2:
        want = ((F.one_hot(yy, C).double() - al / S) ** 2).sum(1) + (al * (S - al) / (S * S * (S + 1))).sum(1)
    else:
        f = torch.log if lt == 0 else torch.digamma
        want = (f(S) - f(al.gather(1, yy[:, None]))).view(-1)
    want.sum().backward()
    return want.detach().numpy(), al.grad.numpy(), S.detach().numpy().reshape(-1)


@pytest.mark.parametrize("lt", range(3))
@pytest.mark.parametrize("ev", range(3))
@pytest.mark.parametrize("nsub", [4, 1])
def test_lane_share_rows_against_float64(H, nsub, ev, lt):
    """row_part / mse_part / row_finish with the classes dealt to nsub lanes, C in {2, 3, 5, 150, 151} (C < nsub: lanes that own
    no class; C mod 4 = 1, 2, 3).  The bound is the one tests/test_evidence_cpu.py holds cls_row to, measured the same way: the
    term to rtol 2e-6 / atol 2e-6, the derivative to 2e-6 of the row's largest element.  An unclassified row (y = -1) gives S
    and |z|_1 only.  With nsub = 1 every field equals cls_row's bit for bit."""
    for C in ROW_C:
        z, y = _rows(C)
        f, d = AE.lane_rows(H, z, y, ev, lt, nsub)
        want, g, S = _float64_rows(z, y, ev, lt)
        cls = y >= 0
        np.testing.assert_allclose(f[:, 4], S, rtol=1e-6, err_msg=f"S, C={C}")
        np.testing.assert_allclose(f[:, 6], np.abs(z.astype(np.float64)).sum(1), rtol=1e-6, err_msg=f"l1, C={C}")
        assert (f[~cls, 5] == 1.0).all()                # alpha_y of a row that is not classified
        err = np.abs(f[cls, 0] - want[cls]) - 2e-6 * np.abs(want[cls])
        print(f"nsub {nsub} ev {ev} lt {lt} C {C}: per max excess over rtol {err.max():.3e} (atol 2e-6); "
              f"derivative max err / scale {(np.abs(d[cls] - g[cls]) / np.abs(g[cls]).max(1, keepdims=True)).max():.3e}")
        np.testing.assert_allclose(f[cls, 0], want[cls], rtol=2e-6, atol=2e-6, err_msg=f"per, C={C}")
        scale = np.abs(g[cls]).max(1, keepdims=True)
        assert float((np.abs(d[cls] - g[cls]) / scale).max()) <= 2e-6, C
        if nsub == 1:
            assert np.array_equal(f.view(np.int32), AE.serial_rows(H, z, y, ev, lt).view(np.int32)), C


# ---- 2. the torch formulation against the fixture
def test_evidence_loss_accepts_mse_in_the_batched_masked_form():
    """EvidenceLoss(loss_type 'mse') on (B,K,C) logits with a mask: err + var per row with one-hot y, summed over the kept rows;
    with_ibm is ignored, as in the reference."""
    from opental_amd.anet.cls_loss import EvidenceLoss
    rs = np.random.RandomState(4)
    z = torch.from_numpy(rs.normal(0, 2, (2, 7, 5))).double()
    tgt = torch.from_numpy(rs.randint(0, 5, (2, 7)))
    mask = torch.from_numpy(rs.rand(2, 7) < 0.6)
    mask[1] = False
    for ev in E.EVIDENCE:
        crit = EvidenceLoss(5, dict(evidence=ev, loss_type='mse'))
        got = crit(z, tgt, mask)
        al = E.torch_evidence(z, ev) + 1
        S = al.sum(-1, keepdim=True)
        per = ((F.one_hot(tgt, 5).double() - al / S) ** 2).sum(-1) + (al * (S - al) / (S * S * (S + 1))).sum(-1)
        np.testing.assert_allclose(got.numpy(), (per * mask).sum(-1).numpy(), rtol=1e-12)
        assert float(got[1]) == 0.0
        with_ibm = EvidenceLoss(5, dict(evidence=ev, loss_type='mse', with_ibm=True, ibm_start=0))
        assert torch.equal(with_ibm(z, tgt, mask), got)
    with pytest.raises(NotImplementedError):
        EvidenceLoss(5, dict(evidence='exp', loss_type='mse', with_ghm=True))
    with pytest.raises(NotImplementedError):
        EvidenceLoss(5, dict(evidence='exp', loss_type='mse', soft_label=0.1))


@pytest.mark.parametrize("name", list(AE.VARIANTS))
def test_host_formulation_matches_reference(fx, name):
    os_head, _ = AE.VARIANTS[name]
    heads = AE.head_outputs(int(fx["seed"]), os_head)
    got = AE.call(AE.criterion(name, epoch=int(fx["epoch"])), heads, AE.targets(fx), weights=tuple(fx["weights"]))
    assert 'AnetDetectionLossFunction' not in got[2]
    AE.check_call(fx, name, got)


def test_fixture_is_what_the_issue_asks_for(fx, golden_dir):
    assert os.path.getsize(os.path.join(golden_dir, "anet_evidence.npz")) <= os.path.getsize(os.path.join(golden_dir, "ablations.npz"))
    assert sorted(n for n, (os_head, _) in AE.VARIANTS.items() if os_head) == sorted(f"{e}_{l}" for e, l in E.PAIRS)
    for name, (os_head, cfg) in AE.VARIANTS.items():
        assert np.isfinite(fx[f"{name}_terms"]).all() and len(fx[f"{name}_terms"]) == (7 if os_head else 5)
        assert all(np.isfinite(fx[f"{name}_grad_{k}"]).all() for k in AE.GRAD_KEYS)
        assert cfg['loss_type'] != 'mse' or 'with_ibm' not in cfg
        assert not os_head or cfg['loss_type'] == 'mse' or cfg['with_ibm']
    assert int(fx["epoch"]) >= AE.IBM['ibm_start']
    for os_head in (True, False):
        h = AE.head_outputs(int(fx["seed"]), os_head)
        assert h["conf"].shape == (2, 189, AE.classes(os_head))
        for k in AE.GRAD_KEYS:
            assert min(float(np.abs(h[k] - e).min()) for e in E.EDGES) >= E.EDGE_MARGIN
            assert not (h[k] <= 0).all(-1).any()        # relu: no row with u = 1
    # sample 1 has no positive anchor: the localisation gradient of its rows is zero
    assert not fx["base_os_grad_loc"][1].any() and fx["base_os_grad_loc"][0].any()


# ---- 3. the routing of the criterion's settings
IOU = dict(iou_aware=True)
ROUTES = [
    # (os_head, cls_loss_type, edl_config, epoch) -> fused_route()
    ((True, 'edl', dict(evidence='exp', loss_type='log', **IOU, **AE.IBM, momentum=0.99, num_bins=50), 12), ('anet_ex', 0, None, True)),
    ((True, 'edl', dict(evidence='exp', loss_type='log', **IOU, **AE.IBM, momentum=0.99, num_bins=50), 3), ('anet_ex', 0, None, False)),
    ((False, 'edl', dict(evidence='exp', loss_type='log'), 12), ('anet_ex', 2, None, False)),        # anet_edl.yaml
    ((False, 'focal', None, 12), ('anet_ex', 3, None, False)),                                       # anet_softmax.yaml
    ((False, 'edl', dict(evidence='exp', loss_type='log', **AE.IBM), 12), ('anet_ev', 2, (0, 0), True)),
    ((False, 'edl', dict(evidence='exp', loss_type='log', **AE.IBM), 3), ('anet_ev', 2, (0, 0), False)),
    ((False, 'edl', dict(evidence='softplus', loss_type='digamma', **AE.IBM), 12), ('anet_ev', 2, (2, 1), True)),
    ((True, 'edl', dict(evidence='relu', loss_type='mse', **AE.IBM), 12), None),                      # mse + IBM: torch
    ((False, 'edl', dict(evidence='softplus', loss_type='mse', **AE.IBM), 3), None),
]
for _e, _l in E.PAIRS:
    _ibm = {} if _l == 'mse' else AE.IBM
    ROUTES.append(((True, 'edl', dict(evidence=_e, loss_type=_l, **IOU, **_ibm), 12),
                   ('anet_ev', 0, (E.EVIDENCE.index(_e), E.LOSS_TYPES.index(_l)), _l != 'mse')))
    ROUTES.append(((False, 'edl', dict(evidence=_e, loss_type=_l), 12),
                   ('anet_ev', 2, (E.EVIDENCE.index(_e), E.LOSS_TYPES.index(_l)), False)))


def _route_criterion(os_head, kind, cfg, epoch):
    from opental_amd.anet.multisegment_loss import MultiSegmentLoss
    crit = MultiSegmentLoss(AE.classes(os_head), 0.6, 1.0, cls_loss_type=kind, edl_config=None if cfg is None else dict(cfg),
                            os_head=os_head)
    if kind == 'edl':
        crit.cls_loss.epoch = epoch
    return crit


@pytest.mark.parametrize("case, want", ROUTES, ids=[f"{'os' if c[0] else 'closed'}-{c[1]}-" + ("" if c[2] is None else
                         f"{c[2]['evidence']}-{c[2]['loss_type']}{'-ibm' if c[2].get('with_ibm') else ''}") + f"-e{c[3]}" for c, _ in ROUTES])
def test_fused_route_table(case, want):
    """fused_route() reads the criterion's settings only: the three shipped configs keep otal_detection_loss_anet_ex, every
    other pair and closed-set IBM go to otal_detection_loss_anet_ev, mse with IBM configured keeps the torch formulation."""
    from opental_amd.anet import multisegment_loss as M
    crit = _route_criterion(*case)
    assert crit.fused_route() == want
    M.FUSED = False
    try:
        assert crit.fused_route() is None               # FUSED = False still forces the torch formulation
    finally:
        M.FUSED = True

    class Dev:                      # what _cls_mode reads of `loc`; host tensors never take a fused entry
        is_cuda, dtype = False, torch.float32
    assert crit._cls_mode(Dev, torch.empty(1, 189, crit.num_classes), AE.priors()) is None


def test_with_ghm_stays_refused():
    for os_head in (True, False):
        with pytest.raises(NotImplementedError, match="with_ghm"):
            _route_criterion(os_head, 'edl', dict(evidence='softplus', loss_type='digamma', with_ghm=True, num_bins=30, momentum=0.85), 12)


def test_the_trainer_capture_key_holds_the_pair_of_this_recipe():
    """anet/train.py builds thumos14.train.DetectorTrainer, whose _capture_key reads evidence / loss_type of criterion.cls_loss:
    the ActivityNet EvidenceLoss carries both attributes."""
    import inspect
    from opental_amd.anet import train as AT
    from opental_amd.thumos14.train import DetectorTrainer
    assert AT.DetectorTrainer is DetectorTrainer
    src = inspect.getsource(DetectorTrainer._capture_key)
    assert "'evidence'" in src and "'loss_type'" in src
    cl = AE.criterion("softplus_digamma").cls_loss
    assert (cl.evidence, cl.loss_type) == ('softplus', 'digamma')


# ---- 4. the entry
def test_anet_ev_is_declared_and_exported(lib):
    txt = open(os.path.join(REPO, "include", "opental_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"\bint\s+otal_detection_loss_anet_ev\s*\(", txt)
    assert hasattr(lib, "otal_detection_loss_anet_ev")
    assert lib.otal_abi_version() == 26


def test_argument_checks_of_anet_ev_do_not_launch(lib):
    """Refusals come before any read or launch: the pointers here are never dereferenced."""
    one = ctypes.c_void_p(16)
    null, shape, unsupported = -1, -2, -7

    def loss(evidence, loss_type, cls_mode=0, ibm=0, K=189, nlev=6, act=one, B=1, lb=one):
        return lib.otal_detection_loss_anet_ev(one, one, one, one, one, act, act, one, one, one, B, K, 150, 1, 768.0, 0.6, lb,
                                               nlev, ibm, 10.0, 1, 0.1, 1.0, cls_mode, 0.25, evidence, loss_type, one,
                                               one, one, None)
    for bad in ((3, 0), (-1, 0), (0, 3), (0, -1)):
        assert loss(*bad) == unsupported, bad
    assert loss(1, 2, ibm=1) == unsupported and loss(0, 2, cls_mode=2, ibm=1) == unsupported        # mse with IBM
    assert loss(1, 1, cls_mode=3) == unsupported and loss(1, 1, cls_mode=1) == unsupported
    assert loss(0, 0, cls_mode=3) == unsupported                # the focal mode is otal_detection_loss_anet_ex's
    assert loss(2, 1, K=1025) == unsupported and loss(2, 1, nlev=9) == unsupported
    # the null and shape checks of _ex
    assert loss(1, 1, act=None) == null                         # the OpenTAL mode needs the actionness maps
    assert loss(1, 1, lb=None) == null and loss(1, 1, cls_mode=2, act=None, lb=None) == null
    assert loss(1, 1, B=0) == shape and loss(1, 1, nlev=0) == shape and loss(1, 1, K=0) == shape
    # otal_detection_loss_anet_ex keeps its refusal of closed-set IBM
    assert lib.otal_detection_loss_anet_ex(one, one, one, one, one, None, None, one, one, one, 1, 189, 151, 1, 768.0, 0.6, one,
                                           6, 1, 10.0, 1, 0.1, 1.0, 2, 0.25, one, one, one, None) == unsupported
