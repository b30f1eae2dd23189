"""Shared by tests/test_anet_evidence_cpu.py, tests/test_anet_evidence_gpu.py and tools/pin_anet_evidence.py: the evidence /
loss-type variants of tests/golden/anet_evidence.npz for the ActivityNet1.3 recipe, their seeded head outputs (B = 2, K = 189:
the recipe's priors with level ids), the g++ harness of the lane-share row functions of opental_amd/csrc/evidence.h, and one
runner of the package's anet MultiSegmentLoss on the fixture's leaves.

Tolerance (the project's rule, ablations_common.tolerances): terms rtol max(2e-5, 4 x the reference's recorded float32-vs-
float64 spread), atol 1e-6; gradients the same factor times the gradient's largest element."""
import ctypes
import os
import subprocess

import numpy as np
import torch

import ablations_common as A
import evidence_common as E
from oracle import afsd_oracle as O
from oracle import arch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CFG = arch.ANET
B = 2
PIOU = 0.6
EPOCH = 12                                      # >= ibm_start: the influence-balanced weight is on where it is configured
IBM = dict(with_ibm=True, ibm_start=10)
W = (1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0)         # lw, cw, lw, cw, ctw, actw, actw of the ActivityNet recipe (--lw 1 --cw 1)
TARGETS = ([[0.10, 0.30, 3.0], [0.45, 0.62, 77.0], [0.70, 0.95, 150.0], [0.05, 0.08, 12.0]],
           [[0.0, 0.005, 2.0]])                 # no prior centre lies in [0, 0.005]: sample 1 has no positive anchor
GRAD_PROBES = 2048                              # conf / prop_conf gradients are stored at strided() positions
GRAD_KEYS = ("conf", "prop_conf")               # the heads whose gradient depends on the evidence function / loss type


def _os_cfg(e, l):
    # log / digamma with the recipe's IBM; the reference's mse_loss applies no weight
    return dict(evidence=e, loss_type=l, iou_aware=True, **({} if l == 'mse' else IBM))


# name -> (os_head, edl_config); C = 150 with os_head, 151 closed set
VARIANTS = {f"{e}_{l}": (True, _os_cfg(e, l)) for e, l in E.PAIRS}
VARIANTS.update({
    "closed_exp_log_ibm": (False, dict(evidence='exp', loss_type='log', **IBM)),
    "closed_softplus_digamma_ibm": (False, dict(evidence='softplus', loss_type='digamma', **IBM)),
    "closed_relu_mse": (False, dict(evidence='relu', loss_type='mse')),
    "closed_relu_log_iou": (False, dict(evidence='relu', loss_type='log', iou_aware=True)),
})


def classes(os_head):
    return 150 if os_head else 151


def priors(dev="cpu"):
    return O.priors_all(CFG).to(dev)


def head_outputs(seed, os_head, batch=B):
    """Synthetic (batch, 189, .) head outputs in the network's ranges: loc in frames (x the level's stride), logits N(0, 2)
    kept off the decision edges of the evidence functions."""
    rs = np.random.RandomState(seed)
    pri = O.priors_all(CFG).numpy()
    K, C = pri.shape[0], classes(os_head)
    stride = np.array([CFG["fpn_strides"][int(l)] for l in pri[:, 1]], np.float32)
    out = dict(loc=(rs.uniform(0.5, 6.0, (batch, K, 2)) * stride[None, :, None]).astype(np.float32),
               conf=E.off_the_edges(rs.normal(0.0, 2.0, (batch, K, C)).astype(np.float32)),
               prop_loc=rs.normal(0.0, 0.3, (batch, K, 2)).astype(np.float32),
               prop_conf=E.off_the_edges(rs.normal(0.0, 2.0, (batch, K, C)).astype(np.float32)),
               center=rs.normal(0.0, 1.0, (batch, K, 1)).astype(np.float32))
    if os_head:
        out["act"] = rs.normal(0.0, 1.0, (batch, K, 1)).astype(np.float32)
        out["prop_act"] = rs.normal(0.0, 1.0, (batch, K, 1)).astype(np.float32)
    return out


def strided(a, n=GRAD_PROBES):
    f = np.asarray(a).reshape(-1)
    return f[::max(1, f.size // n)].copy()


def criterion(name=None, dev="cpu", epoch=EPOCH, cfg=None, os_head=None):
    from opental_amd.anet.multisegment_loss import MultiSegmentLoss
    if cfg is None:
        os_head, cfg = VARIANTS[name]
    crit = MultiSegmentLoss(classes(os_head), PIOU, 1.0, cls_loss_type='edl', edl_config=dict(cfg), os_head=os_head).to(dev)
    crit.cls_loss.epoch = epoch
    return crit


def targets(fx=None, dev="cpu"):
    if fx is None:
        return [torch.tensor(t, dtype=torch.float32, device=dev) for t in TARGETS]
    return [torch.from_numpy(fx["targets_0"]).to(dev), torch.from_numpy(fx["targets_1"]).to(dev)]


def call(crit, heads, tgts, dev="cpu", pri=None, dtype=torch.float32, weights=W):
    """One call of the criterion on fresh leaves: (terms, gradients of sum_i W[i] * term_i, the terms' autograd node name)."""
    ins = {k: torch.from_numpy(v.copy()).to(dev).to(dtype).requires_grad_(True) for k, v in heads.items()}
    pri = priors(dev) if pri is None else pri
    pred = [ins["loc"], ins["conf"], ins["prop_loc"], ins["prop_conf"], ins["center"], pri.to(dtype), ins.get("act"), ins.get("prop_act")]
    terms = crit(pred, [t.to(dev).to(dtype) for t in tgts])
    n = 7 if crit.os_head else 5
    assert crit.os_head or (terms[5] is None and terms[6] is None)
    sum(w * t for w, t in zip(weights, terms[:n])).backward()
    return (np.array([float(t.detach()) for t in terms[:n]]), {k: v.grad.detach().cpu().double().numpy() for k, v in ins.items()},
            type(terms[1].grad_fn).__name__)


def tolerances(fx, name):
    return max(A.TOL, 4 * float(fx[f"{name}_spread_terms"])), max(A.TOL, 4 * float(fx[f"{name}_spread_grads"]))


def check_call(fx, name, got):
    """A call's (terms, grads) against the fixture's record of variant `name`.  conf / prop_conf gradients are stored per
    variant at strided() positions; the other heads' gradients do not depend on the evidence function or the loss type
    (tools/pin_anet_evidence.py asserts it on the reference) and are stored once per head layout (base_os, base_closed)."""
    terms, grads = got[:2]
    rt, rg = tolerances(fx, name)
    print(f"{name}: terms {terms.tolist()} want {fx[f'{name}_terms'].tolist()} rtol {rt:.3g}")
    np.testing.assert_allclose(terms, fx[f"{name}_terms"], rtol=rt, atol=1e-6, err_msg=name)
    base = "base_os" if VARIANTS[name][0] else "base_closed"
    for k, g in grads.items():
        ref, g = (fx[f"{name}_grad_{k}"], strided(g)) if k in GRAD_KEYS else (fx[f"{base}_grad_{k}"], g)
        scale = float(np.abs(ref).max())
        err = float(np.abs(g - ref).max())
        print(f"  grad {k}: max diff {err:.3e}, scale {scale:.3e}, allowed {rg * max(scale, 1e-6):.3e}")
        assert err <= rg * max(scale, 1e-6), (name, k, err, scale)


# ---- the g++ harness of the lane-share row functions (tests/cpu_evidence_lanes.cpp), built as evidence_common.build_harness
def build_harness(out_dir):
    out = os.path.join(str(out_dir), "libcpuevidencelanes.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-std=c++17", "-ffp-contract=off",
                           "-I" + os.path.join(REPO, "opental_amd", "csrc"), os.path.join(HERE, "cpu_evidence_lanes.cpp"), "-o", out])
    return ctypes.CDLL(out)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


FIELDS = ("per", "dS", "dY", "c1", "S", "ay", "l1", "amax")


def lane_rows(H, z, y, evidence, loss_type, nsub):
    """-> (fields (n, 8) in the order of FIELDS, d per / d alpha (n, C)) of row_part / mse_part / row_finish with nsub lanes."""
    z = np.ascontiguousarray(z, np.float32)
    y = np.ascontiguousarray(y, np.int32)
    f, d = np.empty((z.shape[0], 8), np.float32), np.empty_like(z)
    H.cpu_ev_lane_rows(_p(z), _p(y), z.shape[0], z.shape[1], int(evidence), int(loss_type), int(nsub), _p(f), _p(d))
    return f, d


def serial_rows(H, z, y, evidence, loss_type):
    """-> fields (n, 8) of the serial cls_row."""
    z = np.ascontiguousarray(z, np.float32)
    y = np.ascontiguousarray(y, np.int32)
    f = np.empty((z.shape[0], 8), np.float32)
    H.cpu_ev_serial_rows(_p(z), _p(y), z.shape[0], z.shape[1], int(evidence), int(loss_type), _p(f))
    return f
