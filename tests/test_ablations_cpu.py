"""CPU: the THUMOS14 loss ablations (configs/ablations/thumos14_opental_{focal,ghm,ib,hardmib,noMIB,noIoUC,noACT}.yaml) against
tests/golden/ablations.npz, written from the reference by tools/pin_ablations.py -- the package's torch formulation on host
tensors (two consecutive calls at epoch 10, one at epoch 0), the argument checks of otal_detection_loss_ex (no launch), the
reference's yamls written out, and the capture key of the training step across a rule's start epoch."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import yaml

import ablations_common as A


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "ablations.npz"))


@pytest.fixture(scope="module")
def lib():
    from opental_amd.csrc import build
    if not os.path.exists(build.LIB):
        build.build(verbose=False)
    from opental_amd._lib import declare
    return declare(ctypes.CDLL(build.LIB))


def targets_of(fx):
    return [torch.from_numpy(fx["targets_0"]), torch.from_numpy(fx["targets_1"])]


@pytest.mark.parametrize("name", list(A.VARIANTS))
def test_host_formulation_matches_reference(fx, name):
    """Terms, gradients and the state vector of both calls at epoch 10 (the state carries) and of the call at epoch 0."""
    os_head, _ = A.VARIANTS[name]
    heads = A.head_outputs(int(fx["seed"]), 15 if os_head else 16, os_head)
    crit = A.criterion(name, epoch=10)
    for tag in ("call1", "call2"):
        got = A.call(crit, heads, targets_of(fx))
        assert 'DetectionLossFunction' not in got[3]
        A.check_call(fx, name, tag, got, A.grads_tag(fx, name, tag))
    A.check_call(fx, name, "epoch0", A.call(A.criterion(name, epoch=0), heads, targets_of(fx)))


def test_rule_precedence_and_state_buffers():
    from opental_amd.thumos14.cls_loss import EvidenceLoss
    every = dict(A.BASE, with_focal=True, with_ghm=True, with_ibloss=True, ghm_start=10, ib_start=10, **A.IBM)
    assert EvidenceLoss(15, every).reweight() == 'focal'                      # the reference's elif chain, focal ungated
    cl = EvidenceLoss(15, dict(every, with_focal=False, ghm_start=12))
    cl.epoch = 10
    assert cl.reweight() == 'ib'
    cl.epoch = 12
    assert cl.reweight() == 'ghm'
    cl = EvidenceLoss(15, dict(A.BASE, ib_start=10, **A.IBM))
    assert cl.reweight() is None
    # acc_sum is a buffer of the ghm criteria only: every other state dict keeps its keys
    assert set(EvidenceLoss(15, dict(A.BASE, **A.IBM)).state_dict()) == {'weight_accum'}
    ghm = EvidenceLoss(15, A.VARIANTS["ghm"][1])
    assert set(ghm.state_dict()) == {'weight_accum', 'acc_sum'} and ghm.acc_sum.shape == (30,) and not ghm.acc_sum.any()
    with pytest.raises(NotImplementedError):
        EvidenceLoss(15, dict(A.BASE, soft_label=0.1))


def test_ghm_without_a_counted_row_updates_nothing():
    from opental_amd.thumos14.cls_loss import EvidenceLoss
    cl = EvidenceLoss(15, A.VARIANTS["ghm"][1])
    cl.epoch = 10
    cl.acc_sum.copy_(torch.arange(30.0))
    z = torch.randn(6, 15, requires_grad=True)
    loss = cl(z, torch.zeros(6, dtype=torch.long), torch.zeros(6, dtype=torch.bool))
    loss.backward()
    assert float(loss.detach()) == 0.0 and torch.equal(cl.acc_sum, torch.arange(30.0)) and bool(torch.isfinite(z.grad).all())


def test_ib_rows_that_do_not_count_send_no_nan_backwards():
    from opental_amd.thumos14.cls_loss import EvidenceLoss
    cl = EvidenceLoss(15, A.VARIANTS["ib"][1])
    cl.epoch = 10
    z = torch.randn(4, 15)
    z[3] = 0.0                                  # |z|_1 = 0: the weight of this (masked) row is infinite
    z.requires_grad_(True)
    cl(z, torch.zeros(4, dtype=torch.long), torch.tensor([True, True, True, False])).backward()
    assert bool(torch.isfinite(z.grad).all()) and not z.grad[3].any()


def test_ex_entry_exported_and_arguments_checked(lib):
    assert hasattr(lib, "otal_detection_loss_ex")
    assert lib.otal_abi_version() == 26
    one = ctypes.c_void_p(16)     # never dereferenced: argument checks come first

    def ex(cls_mode=0, reweight=0, ibm=0, bins=50, B=1, loc=one, act=one, momentum=0.85):
        return lib.otal_detection_loss_ex(loc, one, one, one, one, act, act, one, one, one, one, B, 126, 15, 1, 256.0, 0.5,
                                          ibm, bins, momentum, 1, cls_mode, 0.25, reweight, 2.0, one, one, one, None)
    assert ex(loc=None) == -1 and ex(cls_mode=0, reweight=2, act=None) == -1      # OTAL_E_NULL
    assert ex(B=0, reweight=1) == -2                                               # OTAL_E_SHAPE
    assert ex(reweight=4) == -7 and ex(reweight=-1) == -7                          # OTAL_E_UNSUPPORTED
    assert ex(cls_mode=1, reweight=1) == -7 and ex(cls_mode=3, reweight=1, act=None) == -7
    assert ex(reweight=2, ibm=1) == -7 and ex(cls_mode=2, reweight=3, ibm=1, act=None) == -7
    assert ex(reweight=2, bins=65) == -7 and ex(bins=65) == -7
    assert ex(reweight=2, momentum=-0.5) == -7
    assert ex(reweight=1, B=17) == -7                                               # B * K beyond the single-workgroup kernel

    def old(cls_mode, ibm, act=one):
        return lib.otal_detection_loss(one, one, one, one, one, act, act, one, one, one, one, 1, 126, 16, 1, 256.0, 0.5,
                                       ibm, 50, 0.99, 1, cls_mode, 0.25, one, one, one, None)
    assert old(2, 1, act=None) == -7            # the existing entry keeps its contract: closed-set EDL without IBM


def test_ex_entry_accepts_ibm_over_a_closed_set(lib):
    """otal_detection_loss_ex(cls_mode 2, ibm_active 1) -- the noACT config -- passes every argument check.  Without a device
    the pointers are placeholders and what comes back is the launch's HIP error, not one of the three argument errors; with a
    device they are real tensors (a launch on placeholders must never reach one) and the call succeeds."""
    if torch.cuda.is_available():
        dev = torch.device("cuda", 0)
        heads = {k: torch.from_numpy(v).to(dev) for k, v in A.head_outputs(3, 16, False, B=1).items()}
        gt = torch.tensor([[[0.1, 0.3, 3.0]]], device=dev)
        keep = [heads[k] for k in ("loc", "conf", "prop_loc", "prop_conf", "center")] + [A.priors(dev)[:, 0].contiguous(), gt,
                torch.ones(1, 1, dtype=torch.uint8, device=dev), torch.ones(50, device=dev), torch.empty(7, device=dev),
                torch.empty(4 * 2 * 126 + 2 * 126 * 16 + 3 * 126, device=dev), torch.empty(126 * 12, device=dev)]
        loc, conf, ploc, pconf, cen, pri, gt_, gv, wacc, losses, grads, scratch = [ctypes.c_void_p(t.data_ptr()) for t in keep]
        assert lib.otal_detection_loss_scratch_floats(1, 126) <= 126 * 12
    else:
        loc = conf = ploc = pconf = cen = pri = gt_ = gv = wacc = losses = grads = scratch = ctypes.c_void_p(16)
    rc = lib.otal_detection_loss_ex(loc, conf, ploc, pconf, cen, None, None, pri, gt_, gv, wacc, 1, 126, 16, 1, 256.0, 0.5,
                                    1, 50, 0.99, 1, 2, 0.25, 0, 0.0, losses, grads, scratch, None)
    assert rc not in (-1, -2, -7), rc
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        assert rc == 0 and bool(torch.isfinite(keep[9][:5]).all())


@pytest.mark.parametrize("name", A.YAMLS)
def test_reference_yaml_builds_model_and_criterion(tmp_path, name):
    from opental_amd.common import config as Cfg
    from opental_amd.thumos14.BDNet import BDNet, model_cfg_from
    from opental_amd.thumos14.multisegment_loss import MultiSegmentLoss
    from opental_amd.thumos14.train import loss_dispatch
    path = tmp_path / f"thumos14_opental_{name}.yaml"
    path.write_text(yaml.safe_dump(A.reference_config(name)))
    config = Cfg.get_config([str(path), "--open_set", "--split", "0"])
    assert loss_dispatch(config) == 'edl'
    md, tr = config['model'], config['training']
    os_head = name != "noACT"
    assert bool(md['os_head']) == os_head
    net = BDNet(in_channels=3, training=False, use_edl=md['use_edl'], cfg=model_cfg_from(config))
    sd = net.state_dict()
    assert tuple(sd["coarse_pyramid_detection.conf_head.conv1d.weight"].shape)[0] == (15 if os_head else 16)
    assert bool([k for k in sd if "actionness" in k]) == os_head
    crit = MultiSegmentLoss(15 if os_head else 16, 0.5, 1.0, cls_loss_type='edl', edl_config=tr['edl_config'], os_head=os_head,
                            act_config=tr['act_config'])
    cl = crit.cls_loss
    crit.cls_loss.epoch = 10
    want = dict(focal='focal', ghm='ghm', ib='ib', hardmib='ibm', noMIB=None, noIoUC='ibm', noACT='ibm')[name]
    assert cl.reweight() == want and crit.iou_aware == (name != "noIoUC")
    crit.cls_loss.epoch = 9
    assert cl.reweight() == ('focal' if name == 'focal' else None)
    assert crit._cls_mode(torch.zeros(1, 126, 2)) is None           # host tensors: the torch formulation
    assert (cl.state() is None) == (name in ("focal", "ib", "noMIB"))
    assert hasattr(cl, 'acc_sum') == (name == "ghm")


class _Tiny(nn.Module):
    def __init__(self):
        super().__init__()
        self.coarse_pyramid_detection = nn.Sequential(nn.Linear(3, 4), nn.Linear(4, 2))
        self.backbone = nn.Sequential(nn.Linear(5, 3), nn.Linear(3, 3))


@pytest.mark.parametrize("name", ["ghm", "ib", "focal", "noMIB"])
def test_capture_key_changes_when_a_rule_starts(name):
    """A captured step bakes `reweight` into the loss launch: the key must differ between epoch 9 and epoch 10 for the gated
    rules, and stay for the ungated / absent ones."""
    from opental_amd.thumos14.train import DetectorTrainer
    crit = A.criterion(name, epoch=9)
    tr = DetectorTrainer(_Tiny(), crit, {}, 1e-4, 1e-4, distributed=False)
    k9 = tr._capture_key()
    crit.cls_loss.epoch = 10
    k10 = tr._capture_key()
    crit.cls_loss.epoch = 11
    assert (k9 != k10) == (name in ("ghm", "ib")) and tr._capture_key() == k10
    st = tr._ibm_state()
    assert (st is crit.cls_loss.acc_sum) if name == "ghm" else st is None
