"""GPU: the ActivityNet1.3 detection loss (csrc/loss.hip: detection_loss_anet_kernel, four lanes per anchor = 256 anchors per
sweep, K <= MAX_KA = 1024) PAST ONE SWEEP.  Every other test of it uses K = 189; here K = 257 (the second sweep is one anchor),
378, 1008 (four sweeps) and 1024 (the limit), with 189 as the control, on the cases of tests/loss_cases.py: every pyramid level
and every 256-anchor sweep of each sample holds positives of both stages (asserted by tests/test_loss_cases_cpu.py)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import loss_cases as LC

pytestmark = pytest.mark.gpu
EDL = dict(evidence='exp', loss_type='log', iou_aware=True, with_ibm=True, ibm_start=10, momentum=0.99, num_bins=50)
CLOSED_EDL = dict(evidence='exp', loss_type='log')
WSUM = (1.0, 0.7, 1.3, 0.9, 1.1, 0.6, 1.2)
NAMES = ("loc", "conf", "prop_loc", "prop_conf", "center", "act", "prop_act")
# instance -> (classes, criterion arguments, epoch, oracle epoch or None)
INSTANCES = {
    "mode0_ibm_on": (150, dict(cls_loss_type='edl', edl_config=EDL, os_head=True), 12, 12),
    "mode0_ibm_off": (150, dict(cls_loss_type='edl', edl_config=EDL, os_head=True), 0, 0),
    "mode2": (151, dict(cls_loss_type='edl', edl_config=dict(CLOSED_EDL, iou_aware=True), os_head=False), 0, None),
    "mode3": (151, dict(cls_loss_type='focal', os_head=False), 0, None),
}
E_UNSUPPORTED = -7


def _crit(inst, dev):
    from opental_amd.anet import multisegment_loss as M
    C, kw, epoch, _ = INSTANCES[inst]
    crit = M.MultiSegmentLoss(C, 0.6, 1.0, **kw).to(dev)
    if hasattr(crit.cls_loss, "epoch"):
        crit.cls_loss.epoch = epoch
    return crit


@functools.lru_cache(maxsize=None)
def _run(inst, K, fused):
    """(terms, gradients of sum WSUM[i] term_i on the CPU, node name) of one call; cached and never modified."""
    from opental_amd.anet import multisegment_loss as M
    dev = torch.device("cuda", 0)
    C = INSTANCES[inst][0]
    heads, targets, priors = LC.anet_inputs(K, C)
    M.FUSED = fused
    try:
        crit = _crit(inst, dev)
        closed = not crit.os_head
        xs = {k: torch.from_numpy(heads[k].copy()).to(dev).requires_grad_(True) for k in NAMES if not (closed and "act" in k)}
        pred = [xs["loc"], xs["conf"], xs["prop_loc"], xs["prop_conf"], xs["center"], torch.from_numpy(priors).to(dev),
                xs.get("act"), xs.get("prop_act")]
        terms = crit(pred, [torch.from_numpy(t).to(dev) for t in targets])
        n = 5 if closed else 7
        assert all(t is None for t in terms[n:])
        sum(w * t for w, t in zip(WSUM, terms[:n])).backward()
        return (np.array([float(t.detach()) for t in terms[:n]]), {k: v.grad.detach().cpu() for k, v in xs.items()},
                type(terms[0].grad_fn).__name__)
    finally:
        M.FUSED = True


@pytest.mark.parametrize("K", list(LC.ANET_LEVELS))
@pytest.mark.parametrize("inst", list(INSTANCES))
def test_fused_anet_loss_past_one_sweep_equals_the_torch_formulation(inst, K):
    """The bounds of test_fused_anet_loss_equals_the_torch_formulation (tests/test_anet_gpu.py): the terms to 2e-5 (of max(1, |term|)),
    every head gradient of the weighted sum to 2e-5 of its scale."""
    t_ref, g_ref, n_ref = _run(inst, K, False)
    t_hip, g_hip, n_hip = _run(inst, K, True)
    assert 'AnetDetectionLossFunction' in n_hip and 'AnetDetectionLossFunction' not in n_ref, (n_ref, n_hip)
    print(f"{inst} K={K}: terms max err {np.abs(t_hip - t_ref).max():.3e}; gradients (of scale) " + ", ".join(
        f"{k} {float((g_hip[k] - g_ref[k]).abs().max()) / max(float(g_ref[k].abs().max()), 1e-30):.2e}" for k in g_ref))
    assert np.isfinite(t_hip).all()
    assert (np.abs(t_hip - t_ref) <= 2e-5 * np.maximum(1.0, np.abs(t_ref))).all(), (t_hip, t_ref)
    for k in g_ref:
        scale = max(float(g_ref[k].abs().max()), 1e-12)
        assert scale > 1e-12, k
        err = float((g_hip[k] - g_ref[k]).abs().max())
        assert err <= 2e-5 * scale + 1e-9, (k, err, scale)


@pytest.mark.parametrize("K", list(LC.ANET_LEVELS))
@pytest.mark.parametrize("inst", ["mode0_ibm_on", "mode0_ibm_off"])
def test_fused_anet_loss_past_one_sweep_equals_the_cpu_oracle(inst, K):
    """cls_mode 0 against oracle.multisegment_loss_anet (the per-sample restatement of the reference) + torch-CPU autograd, the
    same 2e-5 bounds."""
    from oracle import afsd_oracle as O, arch
    t_hip, g_hip, _ = _run(inst, K, True)
    heads, targets, priors = LC.anet_inputs(K, 150)
    cpu = {k: torch.from_numpy(heads[k].copy()).requires_grad_(True) for k in NAMES}
    ref = O.multisegment_loss_anet(dict(cpu, priors=torch.from_numpy(priors)), [torch.from_numpy(t) for t in targets],
                                   cfg=arch.ANET, piou=0.6, epoch=INSTANCES[inst][3])
    sum(w * t for w, t in zip(WSUM, ref)).backward()
    t_ref = np.array([float(t.detach()) for t in ref])
    assert (np.abs(t_hip - t_ref) <= 2e-5 * np.maximum(1.0, np.abs(t_ref))).all(), (t_hip, t_ref)
    for k in NAMES:
        g = cpu[k].grad
        scale = max(float(g.abs().max()), 1e-12)
        assert float((g_hip[k] - g).abs().max()) <= 2e-5 * scale + 1e-9, (k, scale)


def test_more_than_1024_anchors_take_the_torch_formulation():
    """K = 1025: the criterion keeps the torch formulation (the kernel's LDS arrays hold MAX_KA = 1024 anchors) and the C entry
    answers OTAL_E_UNSUPPORTED before it launches anything (the NaN-filled outputs are untouched)."""
    from opental_amd import _lib as L
    from opental_amd.anet import multisegment_loss as M
    from opental_amd.thumos14.multisegment_loss import pad_targets
    dev = torch.device("cuda", 0)
    heads, targets, priors = LC.anet_inputs(1024, 150)
    B, K, C = 2, 1025, 150
    grow = lambda a: np.concatenate([a, a[:, -1:]], 1)          # one more anchor on the last level
    t = {k: torch.from_numpy(grow(heads[k])).to(dev).contiguous() for k in NAMES}
    pri = torch.from_numpy(np.concatenate([priors, priors[-1:]], 0)).to(dev).contiguous()
    tg = [torch.from_numpy(x).to(dev) for x in targets]
    for inst in ("mode0_ibm_on",):
        crit = _crit(inst, dev)
        terms = crit([t["loc"].requires_grad_(True), t["conf"], t["prop_loc"], t["prop_conf"], t["center"], pri, t["act"],
                      t["prop_act"]], tg)
        assert 'AnetDetectionLossFunction' not in type(terms[0].grad_fn).__name__
        assert all(np.isfinite(float(v.detach())) for v in terms)
    gt, valid = pad_targets(tg, dev)
    gv = valid.to(torch.uint8).contiguous()
    lib = L.lib()
    ng = lib.otal_detection_loss_grad_floats(B, K, C)
    nan = lambda n: torch.full((n,), float("nan"), dtype=torch.float32, device=dev)
    losses, grads, scratch = nan(7), nan(ng), nan(8 * B)
    lbs = (ctypes.c_float * 12)(*[float(v) for row in M.bounds for v in row])

    def call(k):
        return lib.otal_detection_loss_anet_ex(*[L.ptr(t[n].detach()) for n in NAMES], L.ptr(pri), L.ptr(gt.contiguous()), L.ptr(gv), B, k,
                                               C, gt.shape[1], 768.0, 0.6, lbs, 6, 1, 10.0, 1, 0.1, 1.0, 0, 0.25,
                                               L.ptr(losses), L.ptr(grads), L.ptr(scratch), L.stream())
    assert call(1025) == E_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool(torch.isnan(losses).all()) and bool(torch.isnan(grads).all()) and bool(torch.isnan(scratch).all())
    assert call(1024) == 0          # the limit itself is accepted (the buffers are larger than it needs)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(losses).all())
