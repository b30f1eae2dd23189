"""GPU: the single-workgroup THUMOS14 detection loss (csrc/loss.hip: detection_loss_kernel, LT = 1024 threads) PAST ONE SWEEP of
its strided loops.  Every other loss test stays at A = B * K <= 1008 anchors, where `for (i = t; i < A; i += LT)` runs once; here
A = 1025 .. 2048 (tests/loss_cases.py, checked under the reference alone by tests/test_loss_cases_cpu.py): every loop takes a
second trip, the bitonic sort of the actionness keys runs with two keys per thread, the histogram segments span samples, and the
launcher crosses the 96 KB switch between the LDS-staged and the unstaged kernel (C = 15: B = 13 -> 14, C = 16: B = 12 -> 13).

Each instance (cls_mode 0 with the IBM EMA off and on, 1, 2, 3, RPL, GCPL and the re-weighting rules 1-4 of the loss ablations) is
compared with the package's torch formulation, modes 0 and 1 also with the CPU oracle, under the bounds those pairings have in
tests/test_loss_gpu.py, test_closed_set_gpu.py, test_rpl_gpu.py and test_ablations_gpu.py: all sums are normalised by a count,
so the bounds do not grow with A."""
import functools
import os

import numpy as np
import pytest
import torch

import ablations_common as AB
import loss_cases as LC

pytestmark = pytest.mark.gpu
W = (1.0, 10.0, 1.0, 10.0, 1.0, 1.0, 1.0)
# the settings of tests/test_loss_gpu.py, test_closed_set_gpu.py and test_rpl_cpu.py
EDL = dict(evidence='exp', loss_type='log', iou_aware=True, with_focal=False, alpha=0.25, gamma=2, with_ibm=True, ibm_start=10,
           momentum=0.99, num_bins=50)
ACT = dict(margin=1.0, weight=0)
CLOSED_EDL = dict(evidence='exp', loss_type='log', soft_label=0, with_focal=False, alpha=0.25, gamma=2)
RPL_VARIANTS = {"rpl": dict(temperature=1, weight_pl=0.1), "gcpl": dict(temperature=1, weight_pl=0.1, gcpl=True)}
E_UNSUPPORTED = -7


def _msl():
    from opental_amd.thumos14 import multisegment_loss as M
    return M


def _edl(dev, epoch):
    crit = _msl().MultiSegmentLoss(15, 0.5, 1.0, cls_loss_type='edl', edl_config=EDL, os_head=True, act_config=ACT).to(dev)
    crit.cls_loss.epoch = epoch
    crit.cls_loss.weight_accum.copy_(torch.linspace(0.5, 1.5, 50))
    return crit


# instance -> (case family, criterion factory, oracle arguments or None, distances instead of logits)
INSTANCES = {
    "mode0_ibm_off": ("open", lambda dev: _edl(dev, 0), ("edl", 0), False),
    "mode0_ibm_on": ("open", lambda dev: _edl(dev, 12), ("edl", 12), False),
    "mode1": ("open", lambda dev: _msl().MultiSegmentLoss(15, 0.5, 1.0, cls_loss_type='focal', edl_config=EDL, os_head=True,
                                                          act_config=ACT).to(dev), ("focal", 0), False),
    "mode2": ("closed", lambda dev: _msl().MultiSegmentLoss(16, 0.5, 1.0, cls_loss_type='edl', edl_config=CLOSED_EDL,
                                                            os_head=False).to(dev), None, False),
    "mode3": ("closed", lambda dev: _msl().MultiSegmentLoss(16, 0.5, 1.0, cls_loss_type='focal', os_head=False).to(dev), None, False),
    "rpl": ("closed", lambda dev: _msl().MultiSegmentLoss(16, 0.5, 1.0, cls_loss_type='rpl',
                                                          rpl_config=dict(RPL_VARIANTS["rpl"])).to(dev), None, True),
    "gcpl": ("closed", lambda dev: _msl().MultiSegmentLoss(16, 0.5, 1.0, cls_loss_type='rpl',
                                                           rpl_config=dict(RPL_VARIANTS["gcpl"])).to(dev), None, True),
    # the re-weighting rules of ablations_common.VARIANTS: RW 1 (focal), 2 (ghm), 3 (ib), and the closed-set IBM rule 4 (noACT)
    "rw1_focal": ("open", lambda dev: AB.criterion("focal", dev, epoch=10), None, False),
    "rw2_ghm": ("open", lambda dev: AB.criterion("ghm", dev, epoch=10), None, False),
    "rw3_ib": ("open", lambda dev: AB.criterion("ib", dev, epoch=10), None, False),
    "rw4_noACT": ("closed", lambda dev: AB.criterion("noACT", dev, epoch=10), None, False),
}
ABLATION = {"rw1_focal": "focal", "rw2_ghm": "ghm", "rw3_ib": "ib", "rw4_noACT": "noACT"}
FULL = (1025, 1134, 1638, 1764, 2016, 2048)
# modes 0 and 1: the whole ladder; modes 2 / 3 / RPL: the rungs test_closed_set_gpu.py does not have, with both sides of the C = 16
# stage switch (12 x 126, 13 x 126); the ablation rules share everything but their weight with mode 0 / 2: the four rungs
LADDER = [(inst, f"open_{a}") for inst in ("mode0_ibm_off", "mode0_ibm_on", "mode1") for a in FULL]
LADDER += [(inst, f"closed_{a}") for inst in ("mode2", "mode3", "rpl", "gcpl") for a in (1025, 1512, 1638, 1764, 2016)]
LADDER += [(inst, f"{INSTANCES[inst][0]}_{a}") for inst in ABLATION for a in LC.RUNGS]


def _state(crit):
    st = getattr(crit.cls_loss, "state", lambda: None)()
    if st is None and hasattr(crit.cls_loss, "weight_accum"):
        st = crit.cls_loss.weight_accum
    return None if st is None else st.detach().cpu().clone()


@functools.lru_cache(maxsize=None)
def _run(inst, case, fused, nostage=0):
    """One call of the criterion on the case: (terms, gradients of sum W[i] term_i on the CPU, state after the call, node name).
    Cached: a (instance, case) pair is evaluated once per form and shared by the tests below; the results are never modified."""
    from opental_amd import _lib as L
    family, make, _, dist = INSTANCES[inst]
    dev = torch.device("cuda", 0)
    heads, targets, priors = LC.thumos_case(case)
    if dist:
        heads = LC.as_distances(heads)
    M = _msl()
    M.FUSED = fused
    L.set_option("OTAL_LOSS_NOSTAGE", nostage)
    try:
        crit = make(dev)
        ins = {k: torch.from_numpy(v.copy()).to(dev).requires_grad_(True) for k, v in heads.items()
               if family == "open" or k not in ("act", "prop_act")}
        out = dict(ins, priors=torch.from_numpy(priors).to(dev))
        out.setdefault("act", None)
        out.setdefault("prop_act", None)
        terms = crit(out, [torch.from_numpy(t).to(dev) for t in targets])
        n = 7 if family == "open" else 5
        assert all(t is None for t in terms[n:])
        sum(w * t for w, t in zip(W, terms[:n])).backward()
        return (np.array([float(t.detach()) for t in terms[:n]]), {k: v.grad.detach().cpu() for k, v in ins.items()},
                _state(crit), type(terms[0].grad_fn).__name__)
    finally:
        M.FUSED = True
        L.set_option("OTAL_LOSS_NOSTAGE", 0)


@functools.lru_cache(maxsize=None)
def _oracle(inst, case):
    from oracle import afsd_oracle as O
    kind, epoch = INSTANCES[inst][2]
    heads, targets, priors = LC.thumos_case(case)
    cpu = {k: torch.from_numpy(v.copy()).requires_grad_(True) for k, v in heads.items()}
    st = O.EvidenceState()
    st.epoch = epoch
    st.weight_accum = torch.linspace(0.5, 1.5, 50)
    ref = O.multisegment_loss(dict(cpu, priors=torch.from_numpy(priors)), [torch.from_numpy(t) for t in targets],
                              cls_loss_type=kind, state=st)
    sum(w * t for w, t in zip(W, ref)).backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in cpu.items()}
    return np.array([float(t.detach()) for t in ref]), grads, st.weight_accum.clone()


def _report(tag, got, want, g_got, g_want):
    rel = np.abs(got - want) / np.maximum(np.abs(want), 1e-30)
    worst = {k: float((g_got[k] - g_want[k]).abs().max()) / max(float(g_want[k].abs().max()), 1e-30) for k in g_want}
    print(f"{tag}: terms max rel {rel.max():.3e}; gradients (of scale) " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))


RAISED = {("rw3_ib", "open_1764"): (4.8e-5, 1.9e-4)}     # (terms rtol, gradient): twice the reference's float64 error, see the docstring


@pytest.mark.parametrize("inst,case", LADDER)
def test_fused_loss_past_one_sweep_matches_torch_formulation(inst, case, golden_dir):
    """Terms, every head gradient of the weighted cost and the IBM / GHM state after the step.  Bounds: rtol 2e-5 / atol 1e-6 on the
    terms, 2e-5 of the gradient's largest element, rtol 1e-5 on the state (2e-5 for the ablations' state, and for `ib` the bound
    ablations_common.tolerances takes from the reference's own float32 spread, as in tests/test_ablations_gpu.py).

    One bound is raised, RAISED below: rw3_ib at open_1764.  ib weighs a row by 1 / (g |z|_1) with g = |1 / alpha_y - C / S|, a
    cancellation that amplifies float32 rounding where g is small.  Measured on an MI355X against the same torch formulation in
    float64 on the CPU (the case has no decision that float64 could take differently): loss_c relative error 2.38e-5 for the
    float32 torch formulation on the GPU, 6.8e-6 for the kernel (kernel vs torch 3.06e-5); conf gradient, of its largest
    element, 9.47e-5 for the torch formulation, 2.64e-5 for the kernel (kernel vs torch 1.21e-4).  The float32 reference is
    further from float64 than the kernel, so the bound of this pair is twice the reference's own error: 4.8e-5 / 1.9e-4.  The
    other three rungs of rw3_ib hold the unraised bounds."""
    l0, g0, s0, n0 = _run(inst, case, False)
    l1, g1, s1, n1 = _run(inst, case, True)
    assert 'DetectionLossFunction' in n1 and 'DetectionLossFunction' not in n0, (n0, n1)
    _report(f"{inst} {case} vs torch", l1, l0, g1, g0)
    rt = rg = 2e-5
    srt = 1e-5
    if inst in ABLATION:
        rt, rg = AB.tolerances(np.load(os.path.join(golden_dir, "ablations.npz")), ABLATION[inst])
        srt = AB.TOL
    rt, rg = RAISED.get((inst, case), (rt, rg))
    assert np.isfinite(l1).all() and np.allclose(l1, l0, rtol=rt, atol=1e-6), (l0, l1)
    if s0 is not None:
        assert torch.allclose(s1, s0, rtol=srt, atol=1e-7), float((s1 - s0).abs().max())
    for k in g0:
        scale = float(g0[k].abs().max())
        assert scale > 0, k
        assert float((g0[k] - g1[k]).abs().max()) <= rg * scale, (k, float((g0[k] - g1[k]).abs().max()), scale)


@pytest.mark.parametrize("inst,case", [(i, c) for i, c in LADDER if INSTANCES[i][2] is not None])
def test_fused_loss_past_one_sweep_matches_cpu_oracle(inst, case):
    """cls_mode 0 and 1 against oracle.multisegment_loss + torch-CPU autograd: rtol 3e-5 / atol 2e-6 on the seven terms, 3e-5 of the
    gradient's scale, 2e-5 on the IBM EMA bins (the bounds of tests/test_loss_gpu.py)."""
    got, g_got, s_got, name = _run(inst, case, True)
    want, g_want, s_want = _oracle(inst, case)
    assert 'DetectionLossFunction' in name
    _report(f"{inst} {case} vs oracle", got, want, g_got, g_want)
    assert np.allclose(got, want, rtol=3e-5, atol=2e-6), (got, want)
    if INSTANCES[inst][2][0] == "edl":
        assert torch.allclose(s_got, s_want, rtol=2e-5, atol=1e-7)
    if inst == "mode0_ibm_on":
        assert not torch.equal(s_got, torch.linspace(0.5, 1.5, 50))         # the bins moved
    for k, g_ref in g_want.items():
        scale = float(g_ref.abs().max())
        assert float((g_got[k] - g_ref).abs().max()) <= 3e-5 * max(scale, 1e-6) + 1e-9, (k, scale)


@pytest.mark.parametrize("inst,case", [("mode0_ibm_on", "open_1025"), ("mode0_ibm_on", "open_1134"), ("mode0_ibm_on", "open_1638"),
                                       ("mode0_ibm_off", "open_1638"), ("mode2", "closed_1025"), ("mode2", "closed_1512"),
                                       ("rpl", "closed_1512"), ("rw2_ghm", "open_1638"), ("rw4_noACT", "closed_1025")])
def test_lds_staged_kernel_changes_no_bit_past_one_sweep(inst, case):
    """test_lds_staged_logits_change_no_bit of tests/test_loss_gpu.py at two trips per thread, up to the last staged size."""
    B, K, C, _ = LC.THUMOS_CASES[case]
    assert B * K * C * 4 <= 96 * 1024          # the default launch of this case IS the staged kernel
    l0, g0, s0, _ = _run(inst, case, True, 1)
    l1, g1, s1, _ = _run(inst, case, True)
    assert np.array_equal(l0, l1), (l0, l1)
    assert (s0 is None and s1 is None) or torch.equal(s0, s1)
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k


# ------------------------------------------------------------------------------------------------- the C entries, called directly
GUARD = 4096
SENTINEL = 0x7fc0beef       # a NaN payload no kernel produces


def _guarded(n, dev):
    """n floats of NaN followed by GUARD floats of the sentinel pattern."""
    buf = torch.full((n + GUARD,), float("nan"), dtype=torch.float32, device=dev)
    buf[n:].view(torch.int32).fill_(SENTINEL)
    return buf


def _raw(inst, case=None, inputs=None):
    """One direct call of the instance's C entry with guarded gradient / scratch buffers: (rc, losses, grads, scratch, state, ng, ns)."""
    from opental_amd import _lib as L
    from opental_amd.thumos14.multisegment_loss import pad_targets
    dev = torch.device("cuda", 0)
    heads, targets, priors = LC.thumos_case(case) if inputs is None else inputs
    if INSTANCES[inst][3]:
        heads = LC.as_distances(heads)
    t = {k: torch.from_numpy(v).to(dev).contiguous() for k, v in heads.items()}
    B, K, C = t["conf"].shape
    gt, valid = pad_targets([torch.from_numpy(x).to(dev) for x in targets], dev)
    gt, gv, pri = gt.contiguous(), valid.to(torch.uint8).contiguous(), torch.from_numpy(priors[:, 0].copy()).to(dev)
    lib = L.lib()
    ng, ns = lib.otal_detection_loss_grad_floats(B, K, C), lib.otal_detection_loss_scratch_floats(B, K)
    assert ng == B * K * (2 * C + 11) and ns == B * K * 12
    losses, grads, scratch = _guarded(7, dev), _guarded(ng, dev), _guarded(ns, dev)
    state = torch.linspace(0.5, 1.5, 50, device=dev)
    tail = [L.ptr(losses), L.ptr(grads), L.ptr(scratch), L.stream()]
    if inst in ("rpl", "gcpl"):
        rc = lib.otal_detection_loss_rpl(*[L.ptr(t[k]) for k in ("loc", "conf", "prop_loc", "prop_conf", "center")], L.ptr(pri),
                                         L.ptr(gt), L.ptr(gv), B, K, C, gt.shape[1], 256.0, 0.5, int(inst == "gcpl"), 1.0,
                                         0.1, 0.0, *tail)
    else:
        mode, ibm = {"mode0_ibm_off": (0, 0), "mode0_ibm_on": (0, 1), "mode1": (1, 0), "mode2": (2, 0), "mode3": (3, 0)}[inst]
        closed = mode >= 2
        p = lambda k: None if (closed and k in ("act", "prop_act")) else L.ptr(t[k])
        rc = lib.otal_detection_loss(*[p(k) for k in ("loc", "conf", "prop_loc", "prop_conf", "center", "act", "prop_act")],
                                     L.ptr(pri), L.ptr(gt), L.ptr(gv), L.ptr(state), B, K, C, gt.shape[1], 256.0, 0.5, ibm, 50,
                                     0.99, int(mode in (0, 2)), mode, 0.25, *tail)
    torch.cuda.synchronize()
    return rc, losses, grads, scratch, state, ng, ns


def _tail_intact(buf, n):
    return bool((buf[n:].view(torch.int32) == SENTINEL).all())


@pytest.mark.parametrize("inst,case", [("mode0_ibm_on", "open_1025"), ("mode0_ibm_on", "open_1638"), ("mode0_ibm_on", "open_1764"),
                                       ("mode0_ibm_on", "open_2048"), ("mode1", "open_2016"), ("mode2", "closed_1512"),
                                       ("mode2", "closed_1638"), ("mode3", "closed_2016"), ("rpl", "closed_1025"),
                                       ("gcpl", "closed_2016")])
def test_kernel_writes_every_gradient_and_nothing_past_its_buffers(inst, case):
    """Gradient and scratch buffers of exactly otal_detection_loss_grad_floats / _scratch_floats, pre-filled with NaN and followed by
    a guard tail: no NaN is left among the gradients (every element is written, the zero slots of the closed-set modes included),
    the seven terms are finite, and the tails still carry their pattern."""
    rc, losses, grads, scratch, _, ng, ns = _raw(inst, case)
    assert rc == 0
    assert _tail_intact(losses, 7) and _tail_intact(grads, ng) and _tail_intact(scratch, ns)
    assert bool(torch.isfinite(losses[:7]).all())
    assert not bool(torch.isnan(grads[:ng]).any()), int(torch.isnan(grads[:ng]).sum())
    assert float(grads[:ng].abs().max()) > 0


@pytest.mark.parametrize("inst,case", [("mode0_ibm_on", "open_2016"), ("mode1", "open_2016"), ("rpl", "closed_2016")])
def test_two_identical_calls_past_one_sweep_are_bitwise_identical(inst, case):
    first, again = _raw(inst, case), _raw(inst, case)
    assert first[0] == 0 and again[0] == 0
    for a, b in zip(first[1:5], again[1:5]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))        # losses, gradients, scratch, state (bit patterns)


def test_more_than_2048_anchors_take_the_torch_formulation():
    """A = 2049: the criterion must not reach the kernel (its LDS arrays hold MAX_A = 2048 anchors), and the C entry refuses with
    OTAL_E_UNSUPPORTED before it launches anything: the state and the NaN-filled outputs are untouched."""
    dev = torch.device("cuda", 0)
    inputs = LC.thumos_inputs(1, (2049,), 15, 3)
    heads, targets, priors = inputs
    for make in (INSTANCES["mode0_ibm_on"][1], INSTANCES["mode1"][1]):
        ins = {k: torch.from_numpy(v.copy()).to(dev).requires_grad_(True) for k, v in heads.items()}
        terms = make(dev)(dict(ins, priors=torch.from_numpy(priors).to(dev)), [torch.from_numpy(t).to(dev) for t in targets])
        assert 'DetectionLossFunction' not in type(terms[0].grad_fn).__name__
        assert all(np.isfinite(float(t.detach())) for t in terms)
    for inst in ("mode0_ibm_on", "mode1", "mode2", "rpl"):
        h = heads if inst in ("mode0_ibm_on", "mode1") else dict(heads, conf=np.pad(heads["conf"], ((0, 0), (0, 0), (0, 1))),
                                                                 prop_conf=np.pad(heads["prop_conf"], ((0, 0), (0, 0), (0, 1))))
        rc, losses, grads, scratch, state, ng, ns = _raw(inst, inputs=(h, targets, priors))
        assert rc == E_UNSUPPORTED, (inst, rc)
        assert bool(torch.isnan(losses[:7]).all()) and bool(torch.isnan(grads[:ng]).all()) and bool(torch.isnan(scratch[:ns]).all())
        assert torch.equal(state, torch.linspace(0.5, 1.5, 50, device=dev))
    # and 2048 itself is accepted
    assert _raw("mode1", "open_2048")[0] == 0
