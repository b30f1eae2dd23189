"""GPU: the backbone tape (I3DFeaturesFunction) against the float64 reference, element by element, zero tolerance.

Every kernel the tape launches is checked alone against float64 elsewhere; what the tape decides itself -- which channel slice of
Z = [h1 | h2 | Y] a launch reads and writes, which folded-BN scale and ReLU mask ride in which data-gradient epilogue, where an
endpoint's external gradient joins the walk, where a bf16-stored region begins and ends -- is checked here on the exactly summable
cases of tests/backbone_tape_cases.py: every sum is exact in fp32 in any order (audited on the CPU,
tests/test_backbone_tape_cases_cpu.py), so every endpoint output, x.grad and weight gradient must EQUAL the reference.  Numbers
are compared: +0 equals -0, a NaN equals nothing.  A wrong slice, scale, mask, tap or tie rule changes an element and fails."""
import numpy as np
import pytest
import torch

import backbone_tape_cases as C

pytestmark = pytest.mark.gpu
MODES = (0, 1)                  # ops.CONV_PRECISION: fp32 operands; bf16 operands (fp32 tensors: HALF_STORAGE off)
_REF = {}


def _reference(label, mode, grads_key=None, grads=None):
    key = (label, mode, grads_key)
    if key not in _REF:
        _REF[key] = C.reference(C.get_case(label), torch.float64, mode, grads=grads)
    return _REF[key]


def _flags(mode):
    """(CONV_PRECISION, HALF_STORAGE, HALF_CHAIN, HALF_ACT_DIRECT) of a mode: 0 / 1 fp32 tensors; 2 the bf16-stored chain;
    3 bf16 storage of a direct layer's output in front of its pool, without the chain."""
    return {0: (0, False, False, False), 1: (1, False, False, False), 2: (1, True, True, False), 3: (1, True, False, True)}[mode]


class _Tape:
    """One run of a plan slice through I3DFeaturesFunction on the device, on the case's tensors."""

    def __init__(self, case, mode, fused_view=False):
        from opental_amd.common import ops
        self.ops, self.case, self.mode = ops, case, mode
        plan, shapes, offs = C.model_plan()
        self.plan, self.offs = plan, offs
        dev = "cuda"
        x_dtype = torch.bfloat16 if (mode >= 2 and case.x_half) else torch.float32      # (the cases' x are bf16 numbers)
        self.scale, self.shift = case.scale.float().to(dev), case.shift.float().to(dev)
        self.x = case.x.detach().to(x_dtype).to(dev).requires_grad_(case.need_dx)
        # weights outside the slice: placeholders whose gradient must come back as None
        self.weights = [torch.zeros(1, device=dev, requires_grad=True) for _ in shapes]
        real = {u: w.detach().float().to(dev) for u, w in case.weights.items()}
        if fused_view:
            # b1a, b2a, b0 of every module back to back in one flat buffer, the order _fused_weight tests for: a zero-copy view
            for st in case.plan:
                if st[0] == "mixed":
                    trio = [st[1] + 1, st[1] + 3, st[1]]
                    flat = torch.cat([real[u].flatten() for u in trio])
                    at = 0
                    for u in trio:
                        n = real[u].numel()
                        real[u] = flat[at:at + n].view(shapes[u])
                        at += n
        for u, w in real.items():
            self.weights[u] = w.requires_grad_(True)

    def run(self, endpoints=None, grads=None, steps=None, x=None):
        """-> dict(outs=, dx=, dw=) as numpy; `grads`: endpoint -> device tensor (any strides), default the case's."""
        from opental_amd.common.i3d_backbone import I3DFeaturesFunction
        ops, case = self.ops, self.case
        endpoints = tuple(endpoints or case.endpoints)
        names = [e.lstrip("=") for e in endpoints]
        if grads is None:
            grads = {e: case.grads[e].float().cuda() for e in names}
        kept = {e: (g, g.clone()) for e, g in grads.items()}
        old = (ops.CONV_PRECISION, ops.HALF_STORAGE, ops.HALF_CHAIN, ops.HALF_ACT_DIRECT)
        ops.CONV_PRECISION, ops.HALF_STORAGE, ops.HALF_CHAIN, ops.HALF_ACT_DIRECT = _flags(self.mode)
        try:
            i0, i1 = steps or (case.i0, case.i1)
            outs = I3DFeaturesFunction.apply(self.x if x is None else x, self.plan[i0:i1], endpoints, self.scale, self.shift, self.offs,
                                             *self.weights)
            # what the tape holds: (kind, dtype of the step's stored output) -- the bf16 tests assert the region from it
            self.held = [(e[0], e[5].dtype if e[0] == "conv" else e[8].dtype if e[0] == "mixed" else None) for e in outs[0].grad_fn.tape]
            torch.autograd.backward(list(outs), [grads[e].to(o.dtype) if grads[e].dtype != o.dtype else grads[e]
                                                 for e, o in zip(names, outs)])
            torch.cuda.synchronize()
        finally:
            ops.CONV_PRECISION, ops.HALF_STORAGE, ops.HALF_CHAIN, ops.HALF_ACT_DIRECT = old
        for e, (g, copy) in kept.items():
            assert torch.equal(g, copy), f"the caller's gradient of {e} was modified"
        return self.collect(dict(zip(names, outs)))

    def forward_only(self, endpoints):
        from opental_amd.common.i3d_backbone import I3DFeaturesFunction
        ops, case = self.ops, self.case
        old = (ops.CONV_PRECISION, ops.HALF_STORAGE, ops.HALF_CHAIN, ops.HALF_ACT_DIRECT)
        ops.CONV_PRECISION, ops.HALF_STORAGE, ops.HALF_CHAIN, ops.HALF_ACT_DIRECT = _flags(self.mode)
        try:
            with torch.no_grad():
                outs = I3DFeaturesFunction.apply(self.x.detach(), self.plan[case.i0:case.i1], tuple(endpoints), self.scale, self.shift,
                                                 self.offs, *[w.detach() for w in self.weights])
            torch.cuda.synchronize()
        finally:
            ops.CONV_PRECISION, ops.HALF_STORAGE, ops.HALF_CHAIN, ops.HALF_ACT_DIRECT = old
        return outs

    def collect(self, outs):
        case = self.case
        for u, w in enumerate(self.weights):
            if u not in case.weights:
                assert w.grad is None, f"weight {u} lies outside the slice: its gradient must be None"
        dw = {}
        for u in case.units:
            assert self.weights[u].grad is not None, f"no gradient for weight {u}"
            dw[u] = self.weights[u].grad.float().cpu().numpy()
        dx = None
        if case.need_dx:
            assert self.x.grad is not None and self.x.grad.dtype == self.x.dtype
            dx = self.x.grad.float().cpu().numpy()
        else:
            assert self.x.grad is None
        return dict(outs={e: o.detach().float().cpu().numpy() for e, o in outs.items()}, dx=dx, dw=dw)


def _same(got, want, what):
    """got (numpy fp32) == want (float64 torch, an fp32 number by the audit), every element."""
    w64 = want.numpy()
    w = w64.astype(np.float32)
    assert np.array_equal(w.astype(np.float64), w64), (what, "the reference is not an fp32 number")
    assert got.shape == w.shape, (what, got.shape, w.shape)
    if not np.array_equal(got, w):
        bad = np.argwhere(~(got == w))
        i = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {w.size} elements differ; first at {i}: got {got[i]!r}, reference {w[i]!r}")


def _check(res, ref, label):
    for e, y in ref["outs"].items():
        if e in res["outs"]:
            _same(res["outs"][e], y, f"{label} output {e}")
    if ref["dx"] is not None:
        _same(res["dx"], ref["dx"], f"{label} dx")
    for u, g in ref["dw"].items():
        _same(res["dw"][u], g, f"{label} dw[{u}]")


def _equal_runs(a, b, what):
    for e in a["outs"]:
        assert np.array_equal(a["outs"][e], b["outs"][e]), (what, e)
    assert (a["dx"] is None) == (b["dx"] is None) and (a["dx"] is None or np.array_equal(a["dx"], b["dx"])), (what, "dx")
    for u in a["dw"]:
        assert np.array_equal(a["dw"][u], b["dw"][u]), (what, "dw", u)


# ---------------------------------------------------------------------------------------------- plan slices
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("label", list(C.FP32_STORED))
def test_slice_equals_the_reference(label, mode):
    res = _Tape(C.get_case(label), mode).run()
    _check(res, _reference(label, mode), f"{label} mode {mode}")


# ---------------------------------------------------------------------------------------------- bf16 storage
@pytest.mark.parametrize("label", list(C.STORED))
def test_bf16_stored_block_equals_the_reference(label):
    """HALF_STORAGE + HALF_CHAIN: the reference rounds what the class docstring says is stored as bf16 (C.reference, mode 2)."""
    case = C.get_case(label)
    t = _Tape(case, 2)
    res = t.run()
    ref = _reference(label, 2)
    _check(res, ref, f"{label} bf16 storage")
    stored = [d for kind, d in t.held if kind in ("conv", "mixed")]
    if label in C.STORED_REGION:
        # the region was really entered: every layer output of the slice is held as bf16, x.grad comes back in x's dtype
        # (collect() asserts it), and the "=" form of the endpoint is the stored tensor itself
        assert stored and all(d == torch.bfloat16 for d in stored), t.held
        assert not case.need_dx or t.x.dtype == torch.bfloat16
        (raw,) = _Tape(case, 2).forward_only(["=" + case.endpoints[0]])
        assert raw.dtype == torch.bfloat16
        _same(raw.float().cpu().numpy(), ref["outs"][case.endpoints[0]], f"{label} '=' output")
    else:
        assert all(d == torch.float32 for d in stored), t.held


@pytest.mark.parametrize("label", list(C.DIRECT))
def test_bf16_layer_output_read_by_its_pool_without_the_chain(label):
    """HALF_ACT_DIRECT on, HALF_CHAIN off: the layer stores bf16, its pool reads that as it is (pool_io1: no conversion seam)."""
    case = C.get_case(label)
    t = _Tape(case, 3)
    res = t.run()
    _check(res, _reference(label, 3), f"{label} direct")
    seam = case.stored[1] > case.stored[0]        # (Conv3d_2c alone stores nothing: see C.DIRECT)
    assert [d for kind, d in t.held if kind == "conv"][-1] == (torch.bfloat16 if seam else torch.float32), t.held
    assert not any(kind == "cvt" for kind, _ in t.held), t.held


# ---------------------------------------------------------------------------------------------- hand-over paths
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("which", (0, 1))
@pytest.mark.parametrize("label", list(C.HANDOVER_PAIRS))
def test_only_one_endpoint_receives_a_gradient(label, which, mode):
    """Two endpoints, a non-zero gradient for the earlier (0) or the later (1) one alone."""
    case = C.get_case(label)
    grads = C.handover_grads(case, f"only{which}")
    res = _Tape(case, mode).run(grads={e: g.float().cuda() for e, g in grads.items()})
    _check(res, _reference(label, mode, f"only{which}", grads), f"{label} only {which} mode {mode}")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("which", (0, 1))
@pytest.mark.parametrize("label", list(C.HANDOVER_PAIRS))
def test_non_dense_gradients_equal_the_dense_run(label, which, mode):
    """One external gradient an expanded stride-0 view (endpoint `which`), the other a permuted view."""
    case = C.get_case(label)
    flat, perm = case.endpoints[which], case.endpoints[1 - which]
    grads = C.handover_grads(case, f"flat{which}")
    ref = _reference(label, mode, f"flat{which}", grads)
    dense = _Tape(case, mode).run(grads={e: g.float().cuda() for e, g in grads.items()})
    _check(dense, ref, f"{label} dense mode {mode}")
    views = {perm: grads[perm].float().cuda().permute(0, 2, 3, 4, 1).contiguous().permute(0, 4, 1, 2, 3),
             flat: grads[flat][:, :, :1, :1, :1].float().cuda().expand(grads[flat].shape)}
    assert not views[perm].is_contiguous() and 0 in views[flat].stride()
    res = _Tape(case, mode).run(grads=views)
    _equal_runs(res, dense, f"{label} views mode {mode}")
    _check(res, ref, f"{label} views mode {mode}")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("label", list(C.HANDOVER_PAIRS))
def test_raw_endpoint_form_equals_the_plain_form(label, mode):
    """"=name" hands an endpoint over as it is stored: in fp32 storage the same tensor and the same walk."""
    case = C.get_case(label)
    res = _Tape(case, mode).run(endpoints=["=" + e for e in case.endpoints])
    _check(res, _reference(label, mode), f"{label} '=' mode {mode}")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("detach", (False, True))
def test_two_nodes_cut_behind_maxpool_4a_equal_one_node(detach, mode):
    """extract_features' split backward by hand: the stem hands "=MaxPool3d_4a_3x3" to a second node; with detach the second node
    reads a leaf twin and the stem runs from stem_out.backward(cut_leaf.grad)."""
    from opental_amd.common.i3d_backbone import I3DFeaturesFunction
    from opental_amd.common import ops
    label = "3c+4a+4b"
    case = C.get_case(label)
    one = _Tape(case, mode).run()
    _check(one, _reference(label, mode), f"{label} mode {mode}")
    t = _Tape(case, mode)
    cut = case.i0 + 2
    g = case.grads[case.endpoints[0]].float().cuda()
    kept = g.clone()
    old = (ops.CONV_PRECISION, ops.HALF_STORAGE, ops.HALF_CHAIN, ops.HALF_ACT_DIRECT)
    ops.CONV_PRECISION, ops.HALF_STORAGE, ops.HALF_CHAIN, ops.HALF_ACT_DIRECT = _flags(mode)
    try:
        (stem_out,) = I3DFeaturesFunction.apply(t.x, t.plan[case.i0:cut], ("=" + t.plan[cut - 1][-1],), t.scale, t.shift, t.offs, *t.weights)
        cut_in = stem_out.detach().requires_grad_(True) if detach else stem_out
        (y,) = I3DFeaturesFunction.apply(cut_in, t.plan[cut:case.i1], case.endpoints, t.scale, t.shift, t.offs, *t.weights)
        y.backward(g)
        if detach:
            stem_out.backward(cut_in.grad)
        torch.cuda.synchronize()
    finally:
        ops.CONV_PRECISION, ops.HALF_STORAGE, ops.HALF_CHAIN, ops.HALF_ACT_DIRECT = old
    assert torch.equal(g, kept)
    two = t.collect({case.endpoints[0]: y})
    _equal_runs(two, one, f"two nodes, detach {detach}, mode {mode}")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("label", ("4b", "3b+3c"))
def test_fused_1x1_weight_as_a_view_and_as_a_copy(label, mode):
    """b1a, b2a, b0 carved back to back from one flat buffer (a zero-copy fused weight) against three separate tensors."""
    from opental_amd.common.i3d_backbone import _fused_weight
    case = C.get_case(label)
    view = _Tape(case, mode, fused_view=True)
    w0 = next(st[1] for st in case.plan if st[0] == "mixed")
    trio = [view.weights[w0 + 1].detach(), view.weights[w0 + 3].detach(), view.weights[w0].detach()]
    assert _fused_weight(*trio).data_ptr() == trio[0].data_ptr(), "the flat layout must give a view"
    copy = _Tape(case, mode)
    trio = [copy.weights[w0 + 1].detach(), copy.weights[w0 + 3].detach(), copy.weights[w0].detach()]
    assert _fused_weight(*trio).data_ptr() != trio[0].data_ptr()
    a, b = view.run(), copy.run()
    _equal_runs(a, b, f"{label} view against copy, mode {mode}")
    _check(a, _reference(label, mode), f"{label} fused view mode {mode}")
