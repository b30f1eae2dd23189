"""Shared by tests/test_ablations_cpu.py and tests/test_ablations_gpu.py: the loss-ablation variants of tools/pin_ablations.py
(restated: the tool needs the reference source tree, the tests must not), its seeded head outputs, the reference's ablation
yamls written out as dicts, and one runner of the package's MultiSegmentLoss on the fixture's leaves."""
import copy

import numpy as np
import torch

from oracle import arch

W = (1.0, 10.0, 1.0, 10.0, 1.0, 1.0, 1.0)        # lw, cw, lw, cw, ctw, actw, actw of the THUMOS14 recipe
ACT = dict(margin=1.0, weight=0)
BASE = dict(evidence='exp', loss_type='log', iou_aware=True, with_focal=False, alpha=0.25, gamma=2)
IBM = dict(with_ibm=True, ibm_start=10, momentum=0.99, num_bins=50)
# name -> (os_head, edl_config): configs/ablations/thumos14_opental_NAME.yaml; ghm0 = ghm with momentum 0 (no EMA)
VARIANTS = {
    "focal": (True, dict(BASE, with_focal=True)),
    "ghm": (True, dict(BASE, with_ghm=True, num_bins=30, momentum=0.85, ghm_start=10)),
    "ghm0": (True, dict(BASE, with_ghm=True, num_bins=30, momentum=0, ghm_start=10)),
    "ib": (True, dict(BASE, with_ibloss=True, ib_start=10)),
    "hardmib": (True, dict(BASE, **dict(IBM, momentum=0))),
    "noMIB": (True, dict(BASE)),
    "noIoUC": (True, dict(BASE, iou_aware=False, **IBM)),
    "noACT": (False, dict(BASE, **IBM)),
}
YAMLS = [n for n in VARIANTS if n != "ghm0"]      # the seven files of the reference
TOL = 2e-5          # terms: rtol (atol 1e-6), as tests/test_closed_set_gpu.py; gradients: of the largest element, as tests/test_loss_gpu.py


def tolerances(fx, name):
    """(term rtol, gradient tolerance relative to the gradient's largest element).  2e-5 unless four times the reference's own
    float32 error (against its float64 run, recorded by the tool) is larger: ib's 1 / (g |z|_1) amplifies rounding."""
    return max(TOL, 4 * float(fx[f"{name}_spread_terms"])), max(TOL, 4 * float(fx[f"{name}_spread_grads"]))


def head_outputs(seed, C, os_head, B=2):
    """tools/pin_ablations.py head_outputs (same seed, same draws)."""
    rs = np.random.RandomState(seed)
    K = sum(arch.level_lengths())
    out = dict(loc=rs.uniform(2.0, 40.0, (B, K, 2)).astype(np.float32),
               conf=rs.normal(0.0, 2.0, (B, K, C)).astype(np.float32),
               prop_loc=rs.normal(0.0, 0.3, (B, K, 2)).astype(np.float32),
               prop_conf=rs.normal(0.0, 2.0, (B, K, C)).astype(np.float32),
               center=rs.normal(0.0, 1.0, (B, K, 1)).astype(np.float32))
    if os_head:
        out["act"] = rs.normal(0.0, 1.0, (B, K, 1)).astype(np.float32)
        out["prop_act"] = rs.normal(0.0, 1.0, (B, K, 1)).astype(np.float32)
    return out


def priors(dev="cpu"):
    return torch.tensor([[(c + 0.5) / t] for t in arch.level_lengths() for c in range(t)], dtype=torch.float32, device=dev)


def criterion(name, dev="cpu", epoch=10):
    from opental_amd.thumos14.multisegment_loss import MultiSegmentLoss
    os_head, cfg = VARIANTS[name]
    crit = MultiSegmentLoss(15 if os_head else 16, 0.5, 1.0, cls_loss_type='edl', edl_config=dict(cfg), os_head=os_head,
                            act_config=dict(ACT)).to(dev)
    crit.cls_loss.epoch = epoch
    return crit


def state_of(crit):
    st = crit.cls_loss.state()
    return np.zeros(0) if st is None else st.detach().cpu().double().numpy()


def call(crit, heads, targets, dev="cpu"):
    """One call of the criterion on fresh leaves: (terms, gradients of sum_i W[i] * term_i, state after the call, the terms'
    autograd node name)."""
    ins = {k: torch.from_numpy(v.copy()).to(dev).requires_grad_(True) for k, v in heads.items()}
    out = dict(ins, priors=priors(dev))
    out.setdefault("act", None)
    out.setdefault("prop_act", None)
    terms = crit(out, [t.to(dev) for t in targets])
    n = 7 if crit.os_head else 5
    assert crit.os_head or (terms[5] is None and terms[6] is None)
    sum(w * t for w, t in zip(W, terms[:n])).backward()
    return (np.array([float(t.detach()) for t in terms[:n]]), {k: v.grad.detach().cpu().numpy() for k, v in ins.items()},
            state_of(crit), type(terms[1].grad_fn).__name__)


def check_call(fx, name, tag, got, grads_tag=None):
    """A call's (terms, grads, state) against the fixture's record `tag` of variant `name`."""
    terms, grads, state = got[:3]
    rt, rg = tolerances(fx, name)
    np.testing.assert_allclose(terms, fx[f"{name}_{tag}_terms"], rtol=rt, atol=1e-6, err_msg=f"{name} {tag}")
    grads_tag = grads_tag or tag
    for k, g in grads.items():
        ref = fx[f"{name}_{grads_tag}_grad_{k}"]
        scale = float(np.abs(ref).max())
        assert float(np.abs(g - ref).max()) <= rg * max(scale, 1e-6), (name, tag, k, float(np.abs(g - ref).max()), scale)
    want = fx[f"{name}_{tag}_state"]
    if want.size:
        np.testing.assert_allclose(state, want, rtol=TOL, atol=1e-7, err_msg=f"{name} {tag} state")


def grads_tag(fx, name, tag):
    """A variant without state gives the same call twice: the tool stored the first call's gradients for both."""
    return tag if f"{name}_{tag}_grad_loc" in fx.files else "call1"


REFERENCE_CONFIG = {
    'dataset': {
        'num_classes': 16,
        'class_info_path': './datasets/thumos14/annotations_open/split_{id:d}/Class_Index_Known.txt',
        'training': {'video_mp4_path': './datasets/thumos14/validation/',
                     'video_info_path': './datasets/thumos14/annotations_open/val_video_info.csv',
                     'video_anno_path': './datasets/thumos14/annotations_open/split_{id:d}/val_Annotation_known.csv',
                     'video_data_path': './datasets/thumos14/validation_npy/',
                     'clip_length': 256, 'clip_stride': 30, 'crop_size': 96},
        'testing': {'video_mp4_path': './datasets/thumos14/test/',
                    'video_info_path': './datasets/thumos14/annotations_open/test_video_info.csv',
                    'video_anno_path': './datasets/thumos14/annotations_open/split_{id:d}/test_Annotation_known.csv',
                    'video_anno_open_path': './datasets/thumos14/annotations_open/test_Annotation_open.csv',
                    'video_data_path': './datasets/thumos14/test_npy/',
                    'crop_size': 96, 'clip_length': 256, 'clip_stride': 128}},
    'model': {'in_channels': 3, 'freeze_bn': True, 'freeze_bn_affine': True, 'use_edl': True, 'evidence': 'exp', 'dropout': 0,
              'os_head': True, 'backbone_model': './models/i3d_models/rgb_imagenet.pt'},
    'training': {'batch_size': 1, 'learning_rate': 1e-5, 'weight_decay': 1e-3, 'max_epoch': 25, 'focal_loss': False,
                 'edl_loss': True, 'edl_config': None, 'act_config': {'margin': 1.0, 'weight': 0},
                 'checkpoint_path': './models/thumos14/opental_{name}/split_{{id:d}}/', 'random_seed': 2020},
    'testing': {'conf_thresh': 0.01, 'top_k': 5000, 'nms_thresh': 0.5, 'nms_sigma': 0.5,
                'checkpoint_path': './models/thumos14/opental_{name}/split_{{id:d}}/checkpoint-latest.ckpt',
                'output_path': './output/opental_{name}/split_{{id:d}}', 'output_json': 'detection_results.json'},
}


def reference_config(name):
    """configs/ablations/thumos14_opental_NAME.yaml of the reference as a dict: thumos14_opental_final.yaml with this variant's
    model.os_head and training.edl_config (and its paths)."""
    cfg = copy.deepcopy(REFERENCE_CONFIG)
    os_head, edl = VARIANTS[name]
    cfg['model']['os_head'] = os_head
    cfg['training']['edl_config'] = dict(edl)
    cfg['training']['checkpoint_path'] = cfg['training']['checkpoint_path'].format(name=name)
    for k in ('checkpoint_path', 'output_path'):
        cfg['testing'][k] = cfg['testing'][k].format(name=name)
    return cfg
