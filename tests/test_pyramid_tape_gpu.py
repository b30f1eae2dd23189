"""The detection half's hand-written tapes, element by element against float64: everything CoarsePyramid does between the
two backbone endpoints and the fourteen output maps -- TrunkFunction / BranchesFunction (thumos14/pyramid_fused.py: gradients
read as channel slices of `cat` buffers, added inside otal_gn_relu_bwd_sum, accumulating data gradients, deferred batch
sums, three lanes), the module-by-module nodes ConvGNReLUFunction / ConvGNReLUPairFunction (common/layers.py), the
ActivityNet layout (one projection, fpn strides, 150-class heads through head_convs_mixed) and the ssl form (level 0 only).

A float64 run takes its own discrete decisions (ReLU signs, pool winners, proposal windows), so the reference is ANCHORED
on the device's forward state (tests/pyramid_tape_ref.py; proven on the CPU by tests/test_pyramid_tape_ref_cpu.py).  The
anchor is collected without touching product code: the fused nodes' `grad_fn.tape` (plus one ops.gn_relu_forward on the
tape's c0 for the Mixed_4f projection before the merge: same kernel, same input, same bits), or wrappers of the two block
nodes' `apply` on the module path.

Tolerance, per compared tensor t:  max|got - ref64| <= 10 * max(E32(t), 2^-23 max|ref64(t)|),  E32 = max|ref32 - ref64| of
the anchored reference on the same anchor (R.distance; never taken from the code under test); 10 is the project's standing
margin for an independent draw with another summation order (tests/test_model_gpu.py:118-125).  (For a tensor of fewer than
16 elements E32 is the largest of three fp32 evaluations of the reference: one draw of a scalar's error says little about its
spread, see R.distance.)  Measured on MI355X: no ratio above 4.5 of the allowed 10.  The smallest wiring error a
tape can make -- one dropped term of a sum, one missed sample -- moves a tensor by 1e-2 of its scale, 10^4 x E32.  No element
is left out.  The early-lane hand-over of the Mixed_4f gradient needs a backbone node as producer and is not covered here;
the distance-head variant stays with tests/test_rpl_gpu.py."""
import numpy as np
import pytest
import torch

from oracle import afsd_oracle as O
from oracle import arch

import pyramid_tape_ref as R

pytestmark = pytest.mark.gpu

torch.set_num_threads(min(16, torch.get_num_threads()))

Q = R.Q
CP = 512                        # ProposalBranch proposal_channels: the concatenation is [roi (CP) | pooled (2 CP) | short (CP)]
BRANCHES = ("loc_proposal_branch", "conf_proposal_branch")
CONFIGS = {                     # name: (layout, batch, fused nodes, ssl form)
    "thumos14-fused": (arch.THUMOS, 2, True, False),
    "thumos14-modules": (arch.THUMOS, 2, False, False),
    "thumos14-ssl": (arch.THUMOS, 2, False, True),
    "anet-modules": (arch.ANET, 1, False, False),
}
_NETS, _REFS = {}, {}


# ----------------------------------------------------------------------------------------------------------- device side
def _setup(name):
    """(cfg, numpy parameters, CPU endpoints, the pyramid on the device, {id(parameter): state-dict key})"""
    if name not in _NETS:
        from opental_amd.common import ops
        cfg, b, _, _ = CONFIGS[name]
        base = "thumos14" if cfg is arch.THUMOS else "anet"
        if base not in _NETS:
            pn = arch.make_params(2020, cfg)
            if cfg is arch.THUMOS:
                from opental_amd.thumos14.BDNet import CoarsePyramid
                pyr = CoarsePyramid([832, 1024], cfg["num_classes"])
            else:
                from opental_amd.anet.BDNet import CoarsePyramid
                pyr = CoarsePyramid(num_cls=cfg["num_classes"], frame_num=cfg["frame_num"])
            pyr.load_state_dict({k[len(Q) + 1:]: torch.from_numpy(v) for k, v in pn.items() if k.startswith(Q + ".")})
            pyr.dirichlet_mode = ops.HEAD_UNCT_MODE['exp']          # as BDNet sets it for use_edl, evidence = 'exp'
            pyr = pyr.cuda().train()
            f4, f5 = R.endpoints(11, b, cfg)
            _NETS[base] = (cfg, pn, f4, f5, pyr, {id(p): f"{Q}.{n}" for n, p in pyr.named_parameters()})
        _NETS[name] = _NETS[base]
    return _NETS[name]


class _Recorder:
    """Wraps the two block nodes' `apply` (module path) and PF.trunk / PF.branches (fused path) for one forward pass."""

    def __init__(self):
        self.blocks, self.trunk, self.branches = {}, None, None

    def __enter__(self):
        from opental_amd.common import layers as LY
        from opental_amd.thumos14 import pyramid_fused as PF
        self.LY, self.PF = LY, PF
        one, pair = LY.ConvGNReLUFunction.apply, LY.ConvGNReLUPairFunction.apply
        self.real = (PF.trunk, PF.branches)

        def one_w(x, w, b, gamma, beta, k, s, sv, levels, groups, eps):
            y = one(x, w, b, gamma, beta, k, s, sv, levels, groups, eps)
            self.blocks[id(w)] = (x, y, levels, s)
            return y

        def pair_w(x0, x1, w0, w1, *rest):
            y0, y1 = pair(x0, x1, w0, w1, *rest)
            self.blocks[id(w0)] = (x0, y0, rest[8], rest[7])
            self.blocks[id(w1)] = (x1, y1, rest[8], rest[7])
            return y0, y1

        def trunk_w(pyramid, feat_dict):
            out = self.real[0](pyramid, feat_dict)
            self.trunk = (out, tuple(feat_dict[ep] for ep in pyramid.projection_inputs))
            return out

        def branches_w(*a):
            self.branches = self.real[1](*a)
            return self.branches
        LY.ConvGNReLUFunction.apply = staticmethod(one_w)
        LY.ConvGNReLUPairFunction.apply = staticmethod(pair_w)
        PF.trunk, PF.branches = trunk_w, branches_w
        return self

    def __exit__(self, *exc):
        del self.LY.ConvGNReLUFunction.apply, self.LY.ConvGNReLUPairFunction.apply
        self.PF.trunk, self.PF.branches = self.real
        return False


def _stride(s):
    return int(s) if isinstance(s, int) else int(s[0])


def _fused_blocks(rec, pyr):
    """{block name: (input, output, level table, stride)} from the two nodes' tapes (read BEFORE backward clears them)."""
    from opental_amd.common import ops
    (loc_feat, conf_feat, frame), (x1, x2) = rec.trunk
    (c0, st0, c1, st1), packed, frame_in, dtape, ptape, tw, (l0, cf0) = loc_feat.grad_fn.tape
    lev = tuple(pyr.levels)
    gn0 = pyr.pyramids[0][1]
    with torch.no_grad():
        p0, _ = ops.gn_relu_forward(c0, gn0.weight, gn0.bias, 32, gn0.eps, True, None)     # the projection before the merge
    w = lambda i: f"{Q}.pyramids.{i}.0.conv{'3' if i < 2 else '1'}d.weight"
    blocks = {w(0): (x1, p0, None, 1), w(1): (x2, packed[:, :, lev[1]:lev[2]], None, 1)}
    for l in range(2, len(lev) - 1):
        blocks[w(l)] = (packed[:, :, lev[l - 1]:lev[l]], packed[:, :, lev[l]:lev[l + 1]], None, 2)
    for i, ci in enumerate((0, 3, 6)):
        blocks[f"{Q}.deconv.{ci}.conv1d.weight"] = (dtape[i][0], dtape[i + 1][0] if i < 2 else frame, None, 1)
    for t, x, ys in (("loc", packed, (l0, loc_feat)), ("conf", packed, (cf0, conf_feat))):
        blocks[f"{Q}.{t}_tower.0.0.conv1d.weight"] = (x, ys[0], lev, 1)
        blocks[f"{Q}.{t}_tower.1.0.conv1d.weight"] = (ys[0], ys[1], lev, 1)
    prop_l, prop_c = rec.branches[0], rec.branches[1]
    cat, pooled_roi, _, lrs = prop_l.grad_fn.tape
    for i, br in enumerate(BRANCHES):
        feat = (loc_feat, conf_feat)[i]
        n = lambda blk: f"{Q}.{br}.{blk}.0.conv1d.weight"
        blocks[n("cur_point_conv")] = (feat, cat[i][:, 3 * CP:], lev, 1)
        blocks[n("lr_conv")] = (feat, lrs[i], lev, 1)
        blocks[n("roi_conv")] = (pooled_roi, cat[i][:, :CP], lev, 1)
        blocks[n("proposal_conv")] = (cat[i], (prop_l, prop_c)[i], lev, 1)
    return blocks


def _forward(name, prec=0, lane=True, need=(True, True), capture=True):
    """One forward pass of CoarsePyramid.forward on leaf endpoints.  -> dict(out={name: device tensor}, leaves={name: leaf},
    blocks={block name: (x, y, levels, stride) on the CPU} and windows (capture=True))."""
    from opental_amd.common import ops
    cfg, pn, f4, f5, pyr, wname = _setup(name)
    _, _, fused, ssl = CONFIGS[name]
    old = (ops.FUSED_PYRAMID, ops.CONV_PRECISION, ops.BRANCH_LANE)
    ops.FUSED_PYRAMID, ops.CONV_PRECISION, ops.BRANCH_LANE = fused, prec, lane
    try:
        feat, leaves = {}, {}
        eps = (("input.f4", f4, need[0]), ("input.f5", f5, need[1])) if f4 is not None else (("input.f5", f5, need[1]),)
        for ep, (key, f, on) in zip(pyr.projection_inputs, eps):
            feat[ep] = f.detach().cuda().requires_grad_(on)
            if on:
                leaves[key] = feat[ep]
        for n, p in pyr.named_parameters():
            leaves[f"{Q}.{n}"] = p
        with _Recorder() as rec:
            res = pyr(feat, ssl=ssl)
            if ssl:
                out = dict(zip(R.SSL_OUTPUTS, res))
            else:
                loc, conf, prop_loc, prop_conf, center, _priors, start, end, slp, elp, scp, ecp, act, prop_act = res[:14]
                unct, prop_unct = res[-1]['unct']
                out = dict(loc=loc, conf=conf, act=act, unct=unct, prop_loc=prop_loc, prop_conf=prop_conf, center=center,
                           prop_act=prop_act, prop_unct=prop_unct, start=start, end=end, start_loc_prop=slp, end_loc_prop=elp,
                           start_conf_prop=scp, end_conf_prop=ecp)
            assert (rec.trunk is not None and rec.branches is not None) == fused, "the path under test did not run"
            r = dict(out=out, leaves=leaves)
            if capture:
                if fused:
                    assert not rec.blocks
                    blocks = _fused_blocks(rec, pyr)
                else:
                    blocks = {wname[i]: v for i, v in rec.blocks.items()}
                r["blocks"] = {n: (x.detach().cpu(), y.detach().cpu(), lv, _stride(s)) for n, (x, y, lv, s) in blocks.items()}
                if not ssl:
                    r["windows"] = tuple(t.cpu() for t in pyr._last_windows)
        return r
    finally:
        ops.FUSED_PYRAMID, ops.CONV_PRECISION, ops.BRANCH_LANE = old


def _lanes_idle():
    from opental_amd.common import ops
    assert not ops.STEP.pending_joins and not ops.STEP.early_results


def _grads(name, cot, subset, **kw):
    """Gradients of sum(out * cot) over `subset` (zeros elsewhere) w.r.t. every parameter and the endpoints that ask for one:
    {name: CPU tensor or None}, and the outputs of that forward pass."""
    from opental_amd.common import ops
    old = (ops.BRANCH_LANE, ops.CONV_PRECISION)
    ops.BRANCH_LANE, ops.CONV_PRECISION = kw.get("lane", True), 0
    try:
        r = _forward(name, capture=False, **kw)
        names = sorted(r["leaves"])
        gs = torch.autograd.grad([r["out"][k] for k in subset], [r["leaves"][n] for n in names],
                                 [cot[k].cuda() for k in subset], allow_unused=True)
        torch.cuda.synchronize()
    finally:
        ops.BRANCH_LANE, ops.CONV_PRECISION = old
    _lanes_idle()
    return {n: None if g is None else g.detach().cpu() for n, g in zip(names, gs)}, {k: v.detach().cpu() for k, v in r["out"].items()}


# ----------------------------------------------------------------------------------------------------------- reference side
def _anchor(name, fwd):
    cfg = CONFIGS[name][0]
    lev = [0] + list(np.cumsum(arch.level_lengths(cfg)))
    blocks = {n: ([y[:, :, lev[l]:lev[l + 1]] for l in range(len(lev) - 1)] if lv is not None else [y])
              for n, (x, y, lv, s) in fwd["blocks"].items()}
    anchor = {"blocks": blocks, "windows": fwd.get("windows")}
    if cfg.get("two_projections", True):
        anchor["merged"] = fwd["blocks"][f"{Q}.loc_tower.0.0.conv1d.weight"][0][:, :, :lev[1]]
    return anchor


def _same_anchor(a, b):
    return (set(a["blocks"]) == set(b["blocks"])
            and all(len(a["blocks"][n]) == len(b["blocks"][n]) and all(torch.equal(s, t) for s, t in zip(a["blocks"][n], b["blocks"][n]))
                    for n in a["blocks"])
            and (a.get("merged") is None) == (b.get("merged") is None)
            and (a.get("merged") is None or torch.equal(a["merged"], b["merged"]))
            and (a["windows"] is None) == (b["windows"] is None)
            and (a["windows"] is None or all(torch.equal(s, t) for s, t in zip(a["windows"], b["windows"]))))


def _reference(name, prec, fwd):
    """The anchored reference of a configuration and operand mode, built once per distinct anchor (the fused and the
    module path run the same kernels on the same operands: one reference serves both)."""
    cfg, b, fused, ssl = CONFIGS[name]
    key = (cfg["name"], ssl, prec)
    anchor = _anchor(name, fwd)
    hit = _REFS.get(key)
    if hit is None or not _same_anchor(hit.anchor, anchor):
        _, pn, f4, f5, _, _ = _setup(name)
        with O.operand_rounding("bf16" if prec else None):
            hit = _REFS[key] = R.Reference(pn, f4, f5, cfg, anchor, ssl)
        hit.cot = R.cotangents(5, hit.r64.out, R.SSL_OUTPUTS if ssl else R.OUTPUTS)
    return hit


def _fp32_reference(name):
    fwd = _forward(name, 0)
    return _reference(name, 0, fwd)


# ----------------------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("prec", [0, 1])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_forward_block_by_block(name, prec):
    """Each block's output against the reference block applied to that block's DEVICE input; the pooled maps and the windows
    bit for bit; every output map against the anchored reference -- fp32 parity mode and bf16 operands."""
    cfg, b, fused, ssl = CONFIGS[name]
    _, pn, _, _, _, _ = _setup(name)
    fwd = _forward(name, prec)
    _lanes_idle()
    lev = [0] + [int(v) for v in np.cumsum(arch.level_lengths(cfg))]
    nblocks = 15 if ssl else 21         # 6 pyramid levels, 3 deconv, 4 tower blocks, 2 x 4 branch blocks (ssl: the two lr_conv only)
    assert len(fwd["blocks"]) == nblocks, sorted(fwd["blocks"])
    with O.operand_rounding("bf16" if prec else None), torch.no_grad():
        P64, P32 = R.params(pn, torch.float64), R.params(pn, torch.float32)
        got, r64, r32 = {}, {}, {}
        for n, (x, y, lv, s) in fwd["blocks"].items():
            got[n] = y
            r64[n] = R.ref_block(P64, n, x.double(), lv, s)
            r32[n] = R.ref_block(P32, n, x, lv, s)
            assert float(y.min()) >= 0 and 0.1 < float((y > 0).float().mean()) < 0.9, n       # a ReLU's output, both signs alive
        R.check(got, r64, R.distance(r64, r32), f"{name} prec {prec} block outputs")
    ref = _reference(name, prec, fwd)
    o64, oe32 = ref.outputs()
    names = R.SSL_OUTPUTS if ssl else R.OUTPUTS
    R.check({k: fwd["out"][k].detach().cpu() for k in names}, {k: o64[k] for k in names}, oe32, f"{name} prec {prec} outputs")
    if ssl:
        return
    seg, fseg = fwd["windows"]
    loc = fwd["out"]["loc"].detach().cpu()
    frame = fwd["blocks"][f"{Q}.deconv.6.conv1d.weight"][1]
    roi = fwd["blocks"][f"{Q}.{BRANCHES[0]}.roi_conv.0.conv1d.weight"][0]
    assert torch.equal(roi, fwd["blocks"][f"{Q}.{BRANCHES[1]}.roi_conv.0.conv1d.weight"][0])      # pooled once, shared
    assert torch.equal(R.bmp(frame.double(), fseg).float(), roi), "frame-level pooled map"
    for i in range(len(lev) - 1):
        sl = slice(lev[i], lev[i + 1])
        s_ref, f_ref = O.proposal_windows(loc[:, sl], lev[i + 1] - lev[i], cfg["frame_num"])        # the rule of test_proposal_windows_bit_exact
        assert torch.equal(seg[:, sl], s_ref) and torch.equal(fseg[:, sl], f_ref), ("windows", i)
        for br in BRANCHES:
            lr = fwd["blocks"][f"{Q}.{br}.lr_conv.0.conv1d.weight"][1][:, :, sl]
            pooled = fwd["blocks"][f"{Q}.{br}.proposal_conv.0.conv1d.weight"][0][:, CP:3 * CP, sl]
            assert torch.equal(R.bmp(lr.double(), seg[:, sl]).float(), pooled), ("pooled map", br, i)


# ----------------------------------------------------------------------------------------------------------- backward
def _cases():
    out = []
    for name, (_, _, _, ssl) in CONFIGS.items():
        out += [(name, "all")] if ssl else [(name, s) for s in R.SUBSETS]
    return out


@pytest.mark.parametrize("name,subset", _cases())
def test_backward_element_by_element(name, subset):
    """Every parameter gradient and both endpoint gradients, fp32 parity mode, for fixed random cotangents on all outputs and
    on subsets with zeros elsewhere: the coarse heads only (no gradient reaches BranchesFunction), the refined heads only, the
    six boundary maps only, start / end only.  A tensor without a path from the subset is absent or exactly zero, as in the
    reference (the ssl form's stride-2 levels)."""
    ssl = CONFIGS[name][3]
    ref = _fp32_reference(name)
    outs = R.SSL_OUTPUTS if ssl else R.SUBSETS[subset]
    got, _ = _grads(name, ref.cot, outs)
    g64, e32 = ref.grads(ref.cot, outs)
    assert set(got) == set(g64)
    alive = [n for n, g in g64.items() if g is not None]
    assert len(alive) >= 8 and all(bool(g64[n].ne(0).any()) for n in alive)
    R.check(got, g64, e32, f"{name} gradients, cotangents on {subset}")


# ----------------------------------------------------------------------------------------------------------- fused only
def _equal(a, b):
    assert set(a) == set(b)
    for n in a:
        assert (a[n] is None) == (b[n] is None), n
        assert a[n] is None or torch.equal(a[n], b[n]), n


def test_fused_nodes_without_the_branch_lane_give_the_same_bits():
    """ops.BRANCH_LANE off: the same launches in one stream.  A lane that reads a tensor too early shows up as a difference."""
    name = "thumos14-fused"
    ref = _fp32_reference(name)
    g_on, o_on = _grads(name, ref.cot, R.OUTPUTS)
    g_off, o_off = _grads(name, ref.cot, R.OUTPUTS, lane=False)
    _equal(o_on, o_off)
    _equal(g_on, g_off)


@pytest.mark.parametrize("need", [(False, True), (True, False), (False, False)])
def test_fused_nodes_keep_their_bits_without_endpoint_gradients(need):
    name = "thumos14-fused"
    ref = _fp32_reference(name)
    g_all, _ = _grads(name, ref.cot, R.OUTPUTS)
    g, _ = _grads(name, ref.cot, R.OUTPUTS, need=need)
    assert set(g_all) - set(g) == {k for k, on in zip(("input.f4", "input.f5"), need) if not on}
    _equal(g, {n: g_all[n] for n in g})


# ----------------------------------------------------------------------------------------------------------- sensitivity
def test_a_dropped_term_of_a_gradient_sum_fails_the_comparison():
    """PF._gn_bwd_adds without the last of its terms (wrong numbers only: one tensor fewer is read)."""
    from opental_amd.thumos14 import pyramid_fused as PF
    name = "thumos14-fused"
    ref = _fp32_reference(name)
    real = PF._gn_bwd_adds
    PF._gn_bwd_adds = lambda adds, *a: real(adds[:-1] if len(adds) > 1 else adds, *a)
    try:
        got, _ = _grads(name, ref.cot, R.OUTPUTS)
    finally:
        PF._gn_bwd_adds = real
    g64, e32 = ref.grads(ref.cot, R.OUTPUTS)
    with pytest.raises(AssertionError):
        R.check(got, g64, e32, "one term of every gradient sum dropped")


def test_a_data_gradient_that_overwrites_instead_of_adding_fails_the_comparison():
    """ops.conv_dgrad ignoring accumulate=True (wrong numbers only: the same buffer, stored instead of added to)."""
    from opental_amd.common import ops
    name = "thumos14-fused"
    ref = _fp32_reference(name)
    real = ops.conv_dgrad

    def plain(*a, **kw):
        kw["accumulate"] = False
        return real(*a, **kw)
    ops.conv_dgrad = plain
    try:
        got, _ = _grads(name, ref.cot, R.OUTPUTS)
    finally:
        ops.conv_dgrad = real
    g64, e32 = ref.grads(ref.cot, R.OUTPUTS)
    with pytest.raises(AssertionError):
        R.check(got, g64, e32, "accumulating data gradients stored instead")
