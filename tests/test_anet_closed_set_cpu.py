"""CPU: the ActivityNet1.3 closed-set Softmax and EDL baselines (os_head false) -- the torch formulation of the loss against
tests/golden/anet_closed_set.npz (tools/pin_anet_closed_set.py), the model config default and the proposal lists of
3- and 4-column Soft-NMS rows."""
import os

import numpy as np
import pytest
import torch

from oracle import afsd_oracle as O
from oracle import arch

C = 151
EDL_CFG = dict(evidence='exp', loss_type='log')
W = (1.0, 1.0, 1.0, 1.0, 1.0)


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


def strided(t, n=4096):
    f = t.detach().reshape(-1)
    return f[::max(1, f.numel() // n)]


@pytest.mark.parametrize("kind", ["focal", "edl"])
def test_torch_formulation_matches_the_reference(fx, kind):
    """MultiSegmentLoss(151, 0.6, 1.0, os_head=False): five terms and the gradients of their weighted sum against the
    reference's anet/multisegment_loss.py on the same inputs; the actionness terms are None as in the reference."""
    from opental_amd.anet.multisegment_loss import MultiSegmentLoss
    crit = MultiSegmentLoss(C, 0.6, 1.0, cls_loss_type=kind, edl_config=EDL_CFG if kind == 'edl' else None, os_head=False)
    assert crit.act_loss is None
    ins = {k: torch.from_numpy(v).requires_grad_(True) for k, v in head_outputs().items()}
    targets = [torch.from_numpy(fx["targets_0"]), torch.from_numpy(fx["targets_1"])]
    terms = crit([ins["loc"], ins["conf"], ins["prop_loc"], ins["prop_conf"], ins["center"], O.priors_all(arch.ANET),
                  None, None], targets)
    assert len(terms) == 7 and terms[5] is None and terms[6] is None
    sum(w * t for w, t in zip(fx["weights"], terms[:5])).backward()
    got = np.array([float(t.detach()) for t in terms[:5]])
    assert np.allclose(got, fx[f"loss_{kind}_terms"], rtol=1e-5, atol=1e-6), (got, fx[f"loss_{kind}_terms"])
    for k, v in ins.items():
        ref = fx[f"loss_{kind}_grad_{k}"]
        scale = max(float(np.abs(ref).max()), 1e-12)
        assert float(np.abs(strided(v.grad).numpy() - ref).max()) <= 1e-5 * scale, k
        assert abs(float(v.grad.double().abs().sum()) - float(fx[f"loss_{kind}_gradsum_{k}"])) <= \
            1e-5 * float(fx[f"loss_{kind}_gradsum_{k}"]) + 1e-9, k


def test_closed_set_criterion_settings():
    """The focal criterion's alpha is the kernel's scalar form (0.25 for the background, 0.75 for the rest); host tensors
    never take the HIP path; the RPL / GCPL losses are not supported."""
    from opental_amd.anet.multisegment_loss import MultiSegmentLoss
    focal = MultiSegmentLoss(C, 0.6, 1.0, cls_loss_type='focal', os_head=False)
    assert focal._focal_alpha0 == 0.25
    al = focal.cls_loss.alpha
    assert float(al[0]) == 0.25 and bool((al[1:] == 0.75).all()) and al.numel() == C
    pri = O.priors_all(arch.ANET)
    assert focal._cls_mode(torch.zeros(1, pri.shape[0], 2), torch.zeros(1, pri.shape[0], C), pri) is None
    with pytest.raises(NotImplementedError):
        MultiSegmentLoss(C, 0.6, 1.0, cls_loss_type='rpl', os_head=False)


def test_model_cfg_without_os_head_is_closed_set():
    """anet/BDNet.py:16: a config without `os_head` builds the closed-set head (151 logits, no actionness); the key keeps
    the OpenTAL head, and BDNet(cfg=None) without a loaded config keeps DEFAULT_MODEL_CFG."""
    from opental_amd.anet.BDNet import DEFAULT_MODEL_CFG, model_cfg_from
    cfg = {'dataset': {'num_classes': 151}, 'model': {'in_channels': 3, 'freeze_bn': True, 'freeze_bn_affine': True,
                                                       'use_edl': True, 'evidence': 'exp'}}
    assert model_cfg_from(cfg)['os_head'] is False and model_cfg_from(cfg)['num_classes'] == 151
    cfg['model']['os_head'] = True
    assert model_cfg_from(cfg)['os_head'] is True
    assert model_cfg_from(None) == DEFAULT_MODEL_CFG and DEFAULT_MODEL_CFG['os_head'] is True
    import yaml
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(repo, "configs", "anet_opental.yaml")) as f:
        assert model_cfg_from(yaml.load(f.read(), Loader=yaml.FullLoader))['os_head'] is True


def test_model_cfg_closed_set_builds_151_logits_and_no_actionness():
    from opental_amd.anet.BDNet import BDNet, DEFAULT_MODEL_CFG
    net = BDNet(training=False, use_edl=True, cfg=dict(DEFAULT_MODEL_CFG, os_head=False))
    cpd = net.coarse_pyramid_detection
    assert net.num_classes == C and not hasattr(cpd, 'actionness_head') and not hasattr(cpd, 'prop_actionness_head')
    assert tuple(cpd.conf_head.conv1d.weight.shape) == (C, 512, 3)
    assert tuple(cpd.prop_conf_head.conv1d.weight.shape) == (C, 512, 1)
    keys = set(net.state_dict())
    params = {k for k in arch.make_params(2020, arch.ANET) if "actionness_head" not in k}
    assert keys == params, sorted(keys ^ params)


@pytest.mark.parametrize("cols", [3, 4, 5])
def test_get_video_prediction_accepts_3_4_and_5_column_rows(cols):
    """anet/test.py:159-200 with use_edl / os_head: the absent uncertainty / actionness columns are written as 0.0; the
    segments are clipped to [0, duration] and the empty ones dropped; class c of the rows is the reference's class c + 1."""
    from opental_amd.anet.test import get_video_prediction
    K, top_k, duration = 3, 4, 50.0
    rows = torch.zeros(K, top_k, cols)
    rows[0, 0, :3] = torch.tensor([-2.0, 10.0, 0.9])
    rows[0, 1, :3] = torch.tensor([60.0, 70.0, 0.8])          # starts after the end of the video: dropped
    rows[2, 0, :3] = torch.tensor([20.0, 55.0, 0.5])
    rows[2, 1, :3] = torch.tensor([21.0, 22.0, 0.0])          # zero score: not a detection
    if cols > 3:
        rows[..., 3] = 0.25
    if cols > 4:
        rows[..., 4] = 0.75
    counts = torch.tensor([2, 0, 2], dtype=torch.int32)
    names = {1: 'a', 2: 'b', 3: 'c'}
    props = get_video_prediction(rows, counts, duration, names)
    assert [p['label'] for p in props] == ['a', 'c']
    assert props[0]['segment'] == [0, 10.0] and props[1]['segment'] == [20.0, 50.0]
    for p in props:
        assert set(p) == {'label', 'score', 'segment', 'uncertainty', 'actionness'}
        assert p['uncertainty'] == (0.25 if cols > 3 else 0.0) and p['actionness'] == (0.75 if cols > 4 else 0.0)


def test_loss_ex_argument_checks_do_not_launch():
    """otal_detection_loss_anet_ex (include/opental_hip.h): act / prop_act may be NULL only in the closed-set modes 2 / 3,
    closed-set EDL has no IBM, and cls_mode 1 (or anything but 0, 2, 3) is not an ActivityNet mode -- all refused on the
    host before anything is read or launched."""
    import ctypes
    from opental_amd.csrc import build
    if not os.path.exists(build.LIB):
        build.build(verbose=False)
    from opental_amd._lib import declare
    lib = declare(ctypes.CDLL(build.LIB))
    p = ctypes.c_void_p(16)                 # never dereferenced: the argument checks come first

    def call(act, cls_mode, ibm_active=0, B=2):
        return lib.otal_detection_loss_anet_ex(p, p, p, p, p, act, act, p, p, p, B, 189, C, 4, 768.0, 0.6, p, 6,
                                               ibm_active, 10.0, 0, 0.1, 1.0, cls_mode, 0.25, p, p, p, None)
    assert call(None, 0) == -1                      # OTAL_E_NULL: the OpenTAL form needs the actionness maps
    assert call(p, 1) == -7 and call(p, 4) == -7 and call(p, -1) == -7        # OTAL_E_UNSUPPORTED
    assert call(None, 2, ibm_active=1) == -7        # closed-set EDL: no influence-balanced weight
    assert call(None, 3, B=0) == -2                 # OTAL_E_SHAPE


def test_activitynet_edl_config_only():
    """The ActivityNet1.3 EvidenceLoss takes the ActivityNet configs (anet_edl.yaml, anet_opental.yaml) for any class count,
    and refuses the options of the THUMOS14 EvidenceLoss it does not have -- soft labels, focal weighting -- even when they
    are off, as the THUMOS14 yamls write them: that config belongs to the other recipe.  RPL / GCPL stay unsupported."""
    from opental_amd.anet.multisegment_loss import MultiSegmentLoss
    anet_opental = dict(evidence='exp', loss_type='log', iou_aware=True, with_ibm=True, ibm_start=10, momentum=0.99,
                        num_bins=50)
    for n, os_head, cfg in ((C, False, EDL_CFG), (201, False, EDL_CFG), (150, True, anet_opental)):
        assert MultiSegmentLoss(n, 0.6, 1.0, cls_loss_type='edl', edl_config=dict(cfg), os_head=os_head).cls_loss.num_cls == n
    thumos_open_edl = dict(evidence='exp', loss_type='log', soft_label=0, with_focal=False, alpha=0.25, gamma=2)
    for os_head in (False, True):
        with pytest.raises(NotImplementedError, match="THUMOS14"):
            MultiSegmentLoss(C, 0.6, 1.0, cls_loss_type='edl', edl_config=thumos_open_edl, os_head=os_head)
        with pytest.raises(NotImplementedError, match="with_focal"):
            MultiSegmentLoss(C, 0.6, 1.0, cls_loss_type='edl', edl_config=dict(EDL_CFG, with_focal=True), os_head=os_head)
        with pytest.raises(NotImplementedError):
            MultiSegmentLoss(C, 0.6, 1.0, cls_loss_type='rpl', os_head=os_head)
