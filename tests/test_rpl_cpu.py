"""CPU: the RPL and GCPL baselines (distance head, closed set) against tests/golden/rpl.npz, written from the reference by
tools/pin_rpl.py -- the float64 checker tests/rpl_ref.py, the package's torch formulation of head and loss on host tensors,
the two reference yamls, the decode's negation and the argument checks of the new C entry points (no launch)."""
import ctypes
import os

import numpy as np
import pytest
import torch
import yaml

import rpl_ref as R
from oracle import arch

C = R.C
VARIANTS = {"rpl": dict(temperature=1, weight_pl=0.1), "gcpl": dict(temperature=1, weight_pl=0.1, gcpl=True)}
PROBE = 1024


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "rpl.npz"))


@pytest.fixture(scope="module")
def lib():
    from opental_amd.csrc import build
    if not os.path.exists(build.LIB):
        build.build(verbose=False)
    from opental_amd._lib import declare
    return declare(ctypes.CDLL(build.LIB))


def head_outputs(B=2, seed=31):
    """loc / prop_loc / center of tools/pin_closed_set.py head_outputs (same seed, same draws; its logits are not used)."""
    rs = np.random.RandomState(seed)
    K = sum(arch.level_lengths())
    out = dict(loc=rs.uniform(2.0, 40.0, (B, K, 2)).astype(np.float32))
    rs.normal(0.0, 2.0, (B, K, C))
    out["prop_loc"] = rs.normal(0.0, 0.3, (B, K, 2)).astype(np.float32)
    rs.normal(0.0, 2.0, (B, K, C))
    out["center"] = rs.normal(0.0, 1.0, (B, K, 1)).astype(np.float32)
    return out


def priors():
    return torch.tensor([[(c + 0.5) / t] for t in arch.level_lengths() for c in range(t)], dtype=torch.float32)


def strided(a, n=PROBE):
    f = np.asarray(a).reshape(-1)
    return f[::max(1, f.size // n)]


def targets_of(fx):
    return [torch.from_numpy(fx["targets_0"]), torch.from_numpy(fx["targets_1"])]


def package_loss(name, targets, heads=None, dev="cpu"):
    """The package's RPLHead + MultiSegmentLoss on the fixture's leaves; (terms, leaves, output dict)."""
    from opental_amd.common.layers import RPLHead
    from opental_amd.thumos14.multisegment_loss import MultiSegmentLoss
    fc, fp, cc, cp, _ = R.seeded_inputs()
    heads = heads or head_outputs()
    ins = {k: torch.from_numpy(heads[k].copy()).to(dev).requires_grad_(True) for k in ("loc", "prop_loc", "center")}
    ins["feat"] = torch.from_numpy(fc.copy()).to(dev).requires_grad_(True)
    ins["prop_feat"] = torch.from_numpy(fp.copy()).to(dev).requires_grad_(True)
    hc, hp = RPLHead(R.D, C).to(dev), RPLHead(R.D, C).to(dev)
    hc.centers.data.copy_(torch.from_numpy(cc))
    hp.centers.data.copy_(torch.from_numpy(cp))
    ins["centers"], ins["prop_centers"] = hc.centers, hp.centers
    tr = lambda y: y.permute(0, 2, 1).contiguous()
    out = dict(loc=ins["loc"], prop_loc=ins["prop_loc"], center=ins["center"], priors=priors().to(dev), act=None, prop_act=None,
               conf=tr(hc(ins["feat"])), prop_conf=tr(hp(ins["prop_feat"])), cls_ctr=hc.centers, prop_cls_ctr=hp.centers,
               ctr_feat=ins["feat"].permute(0, 2, 1), prop_ctr_feat=ins["prop_feat"].permute(0, 2, 1))
    crit = MultiSegmentLoss(C, 0.5, 1.0, cls_loss_type='rpl', rpl_config=dict(VARIANTS[name])).to(dev)
    terms = crit(out, [t.to(dev) for t in targets])
    return terms, ins, out


def check_grads(fx, name, ins, rtol=1e-5):
    for k, v in ins.items():
        g = v.grad.detach().cpu().numpy()
        if k in ("feat", "prop_feat"):
            ref = fx[f"loss_{name}_grad_{k}_probe"]
            np.testing.assert_allclose(strided(g), ref, rtol=rtol, atol=rtol * float(np.abs(ref).max()), err_msg=k)
            np.testing.assert_allclose(g.astype(np.float64).sum(), float(fx[f"loss_{name}_grad_{k}_sum"]), rtol=0,
                                       atol=rtol * float(fx[f"loss_{name}_grad_{k}_abssum"]), err_msg=k)
        else:
            ref = fx[f"loss_{name}_grad_{k}"]
            np.testing.assert_allclose(g, ref, rtol=rtol, atol=rtol * float(np.abs(ref).max()), err_msg=k)


def test_symbols_exported_and_arguments_checked(lib):
    assert hasattr(lib, "otal_rpl_head_fwd") and hasattr(lib, "otal_rpl_head_bwd") and hasattr(lib, "otal_detection_loss_rpl")
    assert lib.otal_abi_version() == 26
    one = ctypes.c_void_p(16)     # never dereferenced: argument checks come first
    fwd = lambda x=one, Cn=16, D=512: lib.otal_rpl_head_fwd(x, one, one, 2, Cn, D, 126, None)
    bwd = lambda g=one, Cn=16, D=512, parts=3: lib.otal_rpl_head_bwd(one, one, g, one, one, 2, Cn, D, 126, parts, None)
    assert fwd(x=None) == -1 and bwd(g=None) == -1                  # OTAL_E_NULL
    assert fwd(Cn=22) == -7 and bwd(Cn=22) == -7                    # OTAL_E_UNSUPPORTED
    assert fwd(D=516) == -7 and bwd(D=516) == -7
    assert fwd(D=520) == -7 and fwd(D=1024) == -7                   # not a multiple of 16; beyond the LDS-resident table
    assert bwd(parts=0) == -2 and bwd(parts=4) == -2

    def loss(loc=one, gcpl=0, B=1):
        return lib.otal_detection_loss_rpl(loc, one, one, one, one, one, one, one, B, 126, C, 1, 256.0, 0.5, gcpl, 1.0,
                                           0.1, 0.0, one, one, one, None)
    assert loss(loc=None) == -1
    assert loss(gcpl=2) == -7
    assert loss(B=17) == -7                                         # B * K beyond the single-workgroup kernel
    assert loss(B=0) == -2


def test_rpl_ref_reproduces_the_golden_head_and_loss(fx):
    fc, fp, cc, cp, g = R.seeded_inputs()
    np.testing.assert_allclose(R.head_fwd(fc, cc), fx["head_dist_f64"], rtol=0, atol=1e-13)
    # the backward restatement against central differences of its own forward, in float64
    dx, dcen = R.head_bwd(fc[:1, :, :3], cc, g[:1, :, :3])
    eps = 1e-6
    for (d, n) in ((0, 0), (7, 2), (511, 1)):
        xp, xm = fc[:1, :, :3].astype(np.float64).copy(), fc[:1, :, :3].astype(np.float64).copy()
        xp[0, d, n] += eps
        xm[0, d, n] -= eps
        num = ((R.head_fwd(xp, cc) - R.head_fwd(xm, cc)) * g[:1, :, :3]).sum() / (2 * eps)
        assert abs(num - dx[0, d, n]) < 1e-8
    cp_, cm_ = cc.astype(np.float64).copy(), cc.astype(np.float64).copy()
    cp_[3, 5] += eps
    cm_[3, 5] -= eps
    num = ((R.head_fwd(fc[:1, :, :3], cp_) - R.head_fwd(fc[:1, :, :3], cm_)) * g[:1, :, :3]).sum() / (2 * eps)
    assert abs(num - dcen[3, 5]) < 1e-8
    heads = head_outputs()
    targets = [fx["targets_0"], fx["targets_1"]]
    cw = float(fx["weights"][1])
    for name, cfg in VARIANTS.items():
        (tc, dxc, dcc), (tp, dxp, dcp) = R.cls_terms_and_grads(fc, fp, cc, cp, heads["loc"], priors().numpy(), targets,
                                                               gcpl=bool(cfg.get("gcpl", False)))
        np.testing.assert_allclose([tc, tp], fx[f"loss_{name}_terms"][[1, 3]], rtol=2e-6)
        for k, got in (("centers", cw * dcc), ("prop_centers", cw * dcp)):
            ref = fx[f"loss_{name}_grad_{k}"]
            np.testing.assert_allclose(got, ref, rtol=1e-5, atol=1e-5 * float(np.abs(ref).max()), err_msg=k)
        for k, got in (("feat", cw * dxc), ("prop_feat", cw * dxp)):
            ref = fx[f"loss_{name}_grad_{k}_probe"]
            np.testing.assert_allclose(strided(got), ref, rtol=1e-5, atol=1e-5 * float(np.abs(ref).max()), err_msg=k)


@pytest.mark.parametrize("name", ["rpl", "gcpl"])
def test_host_formulation_matches_reference(fx, name):
    terms, ins, out = package_loss(name, targets_of(fx))
    assert terms[5] is None and terms[6] is None
    assert float(out["conf"].detach().min()) >= 0.0
    np.testing.assert_allclose([float(t.detach()) for t in terms[:5]], fx[f"loss_{name}_terms"], rtol=2e-5, atol=1e-6)
    sum(float(w) * t for w, t in zip(fx["weights"], terms[:5])).backward()
    check_grads(fx, name, ins)


def test_host_head_matches_the_float64_row(fx):
    """The reference's expanded form on host tensors: within the reference's own fp32 error of the float64 row, times 4."""
    from opental_amd.common.layers import RPLHead
    fc, _, cc, _, _ = R.seeded_inputs()
    h = RPLHead(R.D, C)
    h.centers.data.copy_(torch.from_numpy(cc))
    with torch.no_grad():
        d = h(torch.from_numpy(fc)).numpy()
    err = float(np.abs(d - fx["head_dist_f64"]).max())
    assert err <= 4 * float(fx["head_ref_fp32_err"][0]), err


@pytest.mark.parametrize("name", ["rpl", "gcpl"])
def test_batch_without_positive_anchor_is_finite(fx, name):
    t = torch.from_numpy(fx["targets_1"])           # no prior centre lies inside it
    terms, ins, _ = package_loss(name, [t, t])
    vals = [float(v.detach()) for v in terms[:5]]
    assert np.isfinite(vals).all() and vals[0] == 0.0 and vals[1] > 0.0
    sum(terms[:5]).backward()
    assert all(bool(torch.isfinite(v.grad).all()) for v in ins.values() if v.grad is not None)


RPL_YAML = """
dataset:
  num_classes: 16
  class_info_path: ./datasets/thumos14/annotations_open/split_{id:d}/Class_Index_Known.txt
  training:
    video_mp4_path: ./datasets/thumos14/validation/
    video_info_path: ./datasets/thumos14/annotations_open/val_video_info.csv
    video_anno_path: ./datasets/thumos14/annotations_open/split_{id:d}/val_Annotation_known.csv
    video_data_path: ./datasets/thumos14/validation_npy/
    clip_length: 256
    clip_stride: 30
    crop_size: 96
  testing:
    video_mp4_path: ./datasets/thumos14/test/
    video_info_path: ./datasets/thumos14/annotations_open/test_video_info.csv
    video_anno_path: ./datasets/thumos14/annotations_open/split_{id:d}/test_Annotation_known.csv  # for closed-set eval
    video_anno_open_path: ./datasets/thumos14/annotations_open/test_Annotation_open.csv  # for open-set eval
    video_data_path: ./datasets/thumos14/test_npy/
    crop_size: 96
    clip_length: 256
    clip_stride: 128

model:
  in_channels: 3
  freeze_bn: true
  freeze_bn_affine: true
  use_rpl: true
  backbone_model: ./models/i3d_models/rgb_imagenet.pt

training:
  batch_size: 1
  learning_rate: 1e-5
  weight_decay: 1e-3
  max_epoch: 25
  focal_loss: false
  rpl_loss: true
  rpl_config:
    temperature: 1
    weight_pl: 0.1
%s  checkpoint_path: ./models/thumos14/open_%s/split_{id:d}/
  random_seed: 2020

testing:
  conf_thresh: 0.01
  top_k: 5000
  nms_thresh: 0.5
  nms_sigma: 0.5
  checkpoint_path: ./models/thumos14/open_%s/split_{id:d}/checkpoint-latest.ckpt
  output_path: ./output/open_%s/split_{id:d}
  output_json: detection_results.json
"""


def reference_yaml(name):
    """thumos14_open_rpl.yaml / thumos14_open_gcpl.yaml of the reference, written out (they differ in `gcpl: true` and paths)."""
    return RPL_YAML % ("    gcpl: true\n" if name == "gcpl" else "", name, name, name)


@pytest.mark.parametrize("name", ["rpl", "gcpl"])
def test_reference_yaml_builds_model_and_criterion(tmp_path, name):
    from opental_amd.common import config as Cfg
    from opental_amd.thumos14.BDNet import BDNet, model_cfg_from
    from opental_amd.thumos14.multisegment_loss import MultiSegmentLoss
    from opental_amd.thumos14.test import rpl_flags
    from opental_amd.thumos14.train import loss_dispatch
    path = tmp_path / f"thumos14_open_{name}.yaml"
    path.write_text(reference_yaml(name))
    config = Cfg.get_config([str(path), "--open_set", "--split", "0"])
    assert loss_dispatch(config) == 'rpl' and loss_dispatch(config, as_shipped=True) == 'rpl'
    assert rpl_flags(config) == (True, name == "gcpl")
    net = BDNet(in_channels=3, training=False, use_rpl=config['model']['use_rpl'], cfg=model_cfg_from(config))
    sd = net.state_dict()
    for head in ("conf_head", "prop_conf_head"):
        assert tuple(sd[f"coarse_pyramid_detection.{head}.centers"].shape) == (16, 512)
    assert not [k for k in sd if ".conf_head.conv1d" in k or ".prop_conf_head.conv1d" in k]
    assert not [k for k in sd if "actionness" in k]
    c0 = sd["coarse_pyramid_detection.conf_head.centers"]
    assert 0.05 < float(c0.std()) < 0.15                      # 0.1 * randn, untouched by weight_init
    # a driver that hands the model only the parsed cfg (the cross-dataset one) builds the same heads and learns the decode
    from opental_amd.common.layers import RPLHead
    by_cfg = BDNet(in_channels=3, training=False, cfg=model_cfg_from(config))
    assert isinstance(by_cfg.coarse_pyramid_detection.conf_head, RPLHead) and by_cfg.use_rpl
    assert by_cfg.use_gcpl == (name == "gcpl") and net.use_gcpl == (name == "gcpl")
    crit = MultiSegmentLoss(16, config['training']['piou'], 1.0, cls_loss_type=loss_dispatch(config),
                            rpl_config=config['training']['rpl_config'])
    assert crit.cls_loss_type == 'rpl' and bool(crit.cls_loss.gcpl) == (name == "gcpl")
    assert crit.cls_loss.radius == 0.0 and not list(crit.cls_loss.parameters())      # the untrained radius is a constant


def test_unsupported_settings_raise():
    from opental_amd.common.layers import RPLHead
    from opental_amd.thumos14.BDNet import BDNet, DEFAULT_MODEL_CFG
    from opental_amd.thumos14.multisegment_loss import MultiSegmentLoss
    with pytest.raises(NotImplementedError):
        BDNet(in_channels=3, training=False, use_rpl=True, cfg=dict(DEFAULT_MODEL_CFG, os_head=True))
    with pytest.raises(NotImplementedError):
        RPLHead(512, 16, num_centers=2)
    with pytest.raises(NotImplementedError):
        RPLHead(512, 16)(torch.zeros(1, 512, 4), metric='dot')
    with pytest.raises(NotImplementedError):
        MultiSegmentLoss(15, 0.5, 1.0, cls_loss_type='rpl', rpl_config=dict(VARIANTS["rpl"]), os_head=True)


@pytest.mark.parametrize("name", ["rpl", "gcpl"])
def test_decode_negates_for_gcpl_only(fx, name):
    """rpl_logits feeds the closed-set softmax decode: scores = mean of the two stages' softmax x sigmoid(center), class 0
    dropped -- on host tensors against the reference's conf_scores of both clips."""
    from opental_amd.thumos14.test import rpl_logits
    fc, fp, cc, cp, _ = R.seeded_inputs()
    heads = head_outputs()
    maps = dict(conf=torch.from_numpy(R.head_fwd(fc, cc).transpose(0, 2, 1).astype(np.float32)),
                prop_conf=torch.from_numpy(R.head_fwd(fp, cp).transpose(0, 2, 1).astype(np.float32)),
                center=torch.from_numpy(heads["center"]))
    z = rpl_logits(maps, use_gcpl=name == "gcpl")
    assert (z["conf"] is maps["conf"]) == (name == "rpl")
    if name == "gcpl":
        assert torch.equal(z["conf"], -maps["conf"]) and torch.equal(z["prop_conf"], -maps["prop_conf"])
    score = (torch.softmax(z["conf"], -1) + torch.softmax(z["prop_conf"], -1)) / 2 * torch.sigmoid(z["center"])
    for ci in range(2):
        ref = fx[f"dec_{name}_fus0_score_{ci}"]                 # (C, A), row 0 = background
        np.testing.assert_allclose(score[ci].numpy().T, ref, rtol=1e-5, atol=1e-7)
    other = fx[f"dec_{'rpl' if name == 'gcpl' else 'gcpl'}_fus0_score_0"]
    assert float(np.abs(score[0].numpy().T - other).max()) > 1e-4
