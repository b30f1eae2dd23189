"""Exactly summable inputs of the backbone tape (opental_amd/common/i3d_backbone.py: I3DFeaturesFunction), their float64 reference
and the audit that proves them exact (no GPU code here).

The backbone is convolution, a frozen per-channel affine, ReLU and max-pool.  On small integers, sparse small-integer weights,
power-of-two scales and dyadic shifts every product and every partial sum is an integer multiple of one power of two u and stays
below 2^24 u: it is exact in fp32 in ANY summation order and under any split-K, so the HIP tape must equal the float64
reference element for element -- tests/test_backbone_tape_gpu.py compares with np.array_equal and no tolerance.

  * a case (Case) is a contiguous slice of the product's own plan (InceptionI3d._make_plan(): the model's channel counts, kernel
    sizes and strides) at the model's spatial planes with B = 2 and T = 2..4 inside the plan;
  * reference(): relu(conv(x, w) * scale + shift), O.maxpool3d_same and the branch layout of O.mixed, differentiated by torch
    autograd on the CPU.  mode 1 rounds both operands of every convolution and the gradient operand dz of every backward GEMM
    to bf16 (RNE, explicitly: O._r skips non-fp32 tensors); mode 2 additionally rounds what the bf16-STORED region stores;
  * audit_failures(): for every accumulation of the slice (forward, data gradient and weight gradient of every convolution, the affine
    epilogue, every gradient sum) the shared unit u and sum |a_i| |b_i|, both in float64: the case is valid only if the sum is
    <= 2^24 u.  A condition on the INPUTS, derived, not measured; the value ranges below were tuned until every case holds it;
  * `wrong=`: deliberately wrong variants of the reference (WRONG); tests/test_backbone_tape_cases_cpu.py asserts that each
    changes at least one compared element of every case it applies to, i.e. that the cases would see such a tape error.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import afsd_oracle as O

ONE, THREE = (1, 1, 1), (3, 3, 3)
BATCH = 2
MANTISSA = 24                   # fp32: integers up to 2^24 units are exact
# liveliness thresholds (test_backbone_tape_cases_cpu.py): the least non-zero share of every compared tensor; the other three
# conditions (a pre-activation of exactly 0, a pool window with equal maxima, a border window tying with the padding) are "some"
MIN_NONZERO = 0.25
# the wrong variants: name -> what it breaks
WRONG = {
    "a_swap": "two branch slices of a module output swapped (and with them the gradient's)",
    "b_roll": "the scale vector rolled by one channel in one data-gradient epilogue",
    "c_nomask": "the (Z > 0) mask of a module's input gradient left out",
    "d_unflip": "the temporal taps of a 3x3x3 data gradient unflipped",
    "e_last": "the last maximum instead of the first in a pool",
    "f_rawadd": "an endpoint's external gradient added without its mask and scale",
    "g_nodz": "mode 1: the bf16 rounding of the gradient operand dz left out",
}

_PLAN = None


def model_plan():
    """(plan, weight shapes, channel offsets) of the product's own model."""
    global _PLAN
    if _PLAN is None:
        from opental_amd.common.i3d_backbone import InceptionI3d
        plan, units = InceptionI3d(final_endpoint="Mixed_5c")._make_plan()
        shapes = [tuple(u.conv3d.weight.shape) for u in units]
        offs = [0]
        for s in shapes:
            offs.append(offs[-1] + s[0])
        _PLAN = (plan, shapes, offs)
    return _PLAN


def step_units(step):
    return [step[1]] if step[0] == "conv" else list(range(step[1], step[1] + 6)) if step[0] == "mixed" else []


def _out_channels(step, cin, shapes):
    if step[0] == "conv":
        return shapes[step[1]][0]
    if step[0] == "mixed":
        oc = step[2]
        return oc[0] + oc[2] + oc[4] + oc[5]
    return cin


def bf16_rne(t):
    """Round to nearest even to 8 significant bits, in the tensor's own dtype (float64 included)."""
    m, e = torch.frexp(t)
    return torch.ldexp(torch.round(m * 256.0), e - 8)


def _round_st(t):
    """bf16_rne with a pass-through gradient (t + (r - t) is r exactly: r - t is a difference of neighbours)."""
    return t + (bf16_rne(t) - t).detach() if t.requires_grad else bf16_rne(t)


class Case:
    """steps: endpoint names (or unique prefixes) of a contiguous plan slice; planes: (T, H, W) of the slice's input; endpoints:
    names handed out (default: the last step); nnz: non-zero weights per output channel; exps: the scales are 2^-e, e from this set
    and never equal between neighbouring channels; shift4: shifts are multiples of 1/4 up to this many quarters, both signs."""

    def __init__(self, label, steps, planes, endpoints=None, need_dx=True, seed=1, nnz=24, exps=(1, 2, 3, 4), shift4=3, xmax=3, gmax=2,
                 xfrac=1, x_half=True, stored=None):
        plan, shapes, offs = model_plan()
        names = [st[-1] for st in plan]
        full = lambda s: [n for n in names if n.startswith(s)][0]
        steps = [full(s) for s in steps]
        i0 = names.index(steps[0])
        assert names[i0:i0 + len(steps)] == steps, "a case is a contiguous slice of the plan"
        self.label, self.i0, self.i1 = label, i0, i0 + len(steps)
        self.plan = plan[self.i0:self.i1]
        self.endpoints = tuple(full(e) for e in (endpoints or [steps[-1]]))
        self.need_dx = need_dx
        # modes 2 / 3 only: is x handed over as a bf16 tensor, and which steps [a, b) of the slice lie in the bf16-stored region
        self.x_half, self.stored = x_half, stored or (0, len(steps))
        self.units = [u for st in self.plan for u in step_units(st)]
        # channels in front of the slice: the model's
        cin = 3
        for st in plan[:i0]:
            cin = _out_channels(st, cin, shapes)
        self.x_shape = (BATCH, cin) + tuple(planes)
        rs = np.random.RandomState(seed)
        # x: small integers (xfrac > 1: multiples of 1/xfrac, operands that need more than 8 bits where a conv reads x itself)
        self.x = torch.from_numpy(rs.randint(-xmax * xfrac, xmax * xfrac + 1, self.x_shape).astype(np.float64) / xfrac)
        self.weights = {}
        for u in self.units:
            shp = shapes[u]
            fan = int(np.prod(shp[1:]))
            n = min(nnz, fan)
            idx = np.argsort(rs.rand(shp[0], fan), axis=1)[:, :n]
            val = rs.choice([-1.0, 1.0, -2.0, 2.0], size=(shp[0], n), p=[0.4, 0.4, 0.1, 0.1])
            w = np.zeros((shp[0], fan))
            np.put_along_axis(w, idx, val, axis=1)
            self.weights[u] = torch.from_numpy(w.reshape(shp))
        # scale / shift over the channels of ALL units (the tape slices them by offs): neighbours never share a scale
        C = offs[-1]
        e = np.empty(C, np.int64)
        e[0] = 0
        for c in range(1, C):
            e[c] = (e[c - 1] + rs.randint(1, len(exps))) % len(exps) if len(exps) > 1 else 0
        self.scale = torch.from_numpy(np.ldexp(1.0, -np.asarray(exps)[e]))
        self.shift = torch.from_numpy(rs.randint(-shift4, shift4 + 1, C).astype(np.float64) / 4.0)
        self.offs = offs
        # one integer upstream gradient per endpoint
        shape, self.out_shapes = self.x_shape, {}
        for st in self.plan:
            k, s = (st[2], st[3]) if st[0] == "conv" else (st[1], st[2]) if st[0] == "pool" else (ONE, ONE)
            shape = (BATCH, _out_channels(st, shape[1], shapes)) + tuple(-(-n // q) for n, q in zip(shape[2:], s))
            self.out_shapes[st[-1]] = shape
        self.grads = {e: torch.from_numpy(rs.randint(-gmax, gmax + 1, self.out_shapes[e]).astype(np.float64)) for e in self.endpoints}

    def __repr__(self):
        return self.label


# ---------------------------------------------------------------------------------------------- the reference
class _Tap(torch.autograd.Function):
    """Identity; the backward pass rounds the gradient to bf16 (rnd) and / or notes it in `rec`."""
    @staticmethod
    def forward(ctx, t, rec, rnd):
        ctx.rec, ctx.rnd = rec, rnd
        return t.view_as(t)

    @staticmethod
    def backward(ctx, g):
        if ctx.rnd:
            g = bf16_rne(g)
        if ctx.rec is not None:
            ctx.rec["g"] = g.detach()
        return g, None, None


def _tap(t, rec=None, rnd=False):
    return _Tap.apply(t, rec, rnd) if t.requires_grad and (rec is not None or rnd) else t


class _UnflippedDgradConv(torch.autograd.Function):
    """conv3d whose data gradient reads the temporal taps in the forward's order (wrong variant d)."""
    @staticmethod
    def forward(ctx, xp, w, s):
        ctx.save_for_backward(xp, w)
        ctx.s = s
        return F.conv3d(xp, w, None, stride=s)

    @staticmethod
    def backward(ctx, dz):
        xp, w = ctx.saved_tensors
        return (torch.nn.grad.conv3d_input(xp.shape, w.flip(2), dz, stride=ctx.s),
                torch.nn.grad.conv3d_weight(xp, w.shape, dz, stride=ctx.s), None)


def windows(x, k, s):
    """(windows (B,C,To,Ho,Wo,kvol) of the zero-padded x in the scan order t, h, w; the same of a 0/1 map that marks padding)."""
    un = lambda t: O._pad3(t, k, s).unfold(2, k[0], s[0]).unfold(3, k[1], s[1]).unfold(4, k[2], s[2]).flatten(5)
    return un(x), un(torch.ones_like(x).detach()) == 0


def pool_pick(x, k, s, last=False):
    """MaxPool3dSamePadding by explicit windows: the first (or, wrong, the last) maximum of the zero-padded window wins."""
    win, _ = windows(x, k, s)
    top = win.detach().max(-1, keepdim=True).values
    idx = torch.arange(win.shape[-1]).expand_as(win)
    eq = win.detach() == top
    pick = torch.where(eq, idx, -1).max(-1, keepdim=True).values if last else torch.where(eq, idx, win.shape[-1]).min(-1, keepdim=True).values
    return win.gather(-1, pick).squeeze(-1)


class _Run:
    def __init__(self, case, dtype, mode, wrong, audit, live):
        self.case, self.dtype, self.mode, self.wrong, self.audit, self.live = case, dtype, mode, wrong, audit, live
        self.applied = wrong is None
        self.storing = False
        self.scale, self.shift = case.scale.to(dtype), case.shift.to(dtype)
        self.w = {u: w.detach().clone().to(dtype).requires_grad_(True) for u, w in case.weights.items()}

    def take(self, name):
        """True once: the first site where the wrong variant `name` applies."""
        if self.wrong == name and not self.applied:
            self.applied = True
            return True
        return False

    def store(self, t, tag):
        """An activation of the bf16-STORED region (mode 2): kept as bf16, and so is its gradient (rounded once)."""
        if self.storing:
            t = _tap(_round_st(t), None, True)
        if self.audit is not None:
            self.audit.append(dict(kind="stored", tag=tag, t=t.detach()))
        return t

    def conv(self, x, u, k, s, consumed):
        xr, wr = (_round_st(x), _round_st(self.w[u])) if self.mode else (x, self.w[u])
        xp = O._pad3(xr, k, s)
        if tuple(k) == THREE and xr.requires_grad and self.take("d_unflip"):
            z = _UnflippedDgradConv.apply(xp, wr, tuple(s))
        else:
            z = F.conv3d(xp, wr, None, stride=tuple(s))
        rec = None
        if self.audit is not None:
            rec = dict(kind="conv", tag=f"unit{u}", x=xr.detach(), w=wr.detach(), k=k, s=s, g=None, dx=xr.requires_grad)
            self.audit.append(rec)
        nodz = self.mode and self.wrong == "g_nodz"
        if nodz:
            self.applied = True
        z = _tap(z, rec, bool(self.mode) and not nodz)
        o0, o1 = self.case.offs[u], self.case.offs[u + 1]
        sc, sh = self.scale[o0:o1].view(1, -1, 1, 1, 1), self.shift[o0:o1].view(1, -1, 1, 1, 1)
        pre = z * sc + sh
        if consumed and self.take("b_roll"):
            pre = pre.detach() + (z - z.detach()) * sc.roll(1, 1)
        if self.audit is not None:
            self.audit.append(dict(kind="affine", tag=f"unit{u}", z=z.detach(), sc=sc, sh=sh))
        if self.live is not None:
            self.live["pre_zero"] += int((pre.detach() == 0).sum())
        return F.relu(pre), pre, z

    def pool(self, x, k, s, tag):
        if self.live is not None:
            win, pad = windows(x.detach(), k, s)
            top = win.max(-1, keepdim=True).values
            eq = win == top
            self.live["pool_ties"] += int((eq.sum(-1) > 1).sum())
            self.live["pad_ties"] += int(((eq & pad).any(-1) & (eq & ~pad).any(-1)).sum())
            self.live["padded"] += int(pad.any())
            self.live["pools"] += 1
        if x.requires_grad and self.take("e_last"):
            y = pool_pick(x, k, s, last=True)
        else:
            y = O.maxpool3d_same(x, k, s)
        if self.audit is not None:
            rec = dict(kind="pool", tag=tag, k=k, s=s, g=None)
            self.audit.append(rec)
            y = _tap(y, rec)
        return y

    def mixed(self, x, w0, oc, name):
        """The branch layout of O.mixed: [b0 | b1b(b1a) | b2b(b2a) | b3b(pool)]."""
        recp = None
        xq = x
        if self.storing:
            # the fused 1x1 data gradient is stored as bf16, the branch pool's backward is added to it and the sum rounded once
            # more (the second rounding is the tap of store() on x)
            xq = _tap(x, None, True)
        xpool = x
        if self.audit is not None:
            recp = dict(kind="part", g=None)
            xpool = _tap(x, recp)
        n0 = len(self.audit) if self.audit is not None else 0
        b0 = self.conv(xq, w0, ONE, ONE, False)
        h1 = self.conv(xq, w0 + 1, ONE, ONE, True)
        h1y = self.store(h1[0], f"{name}.h1")
        b1 = self.conv(h1y, w0 + 2, THREE, ONE, False)
        h2 = self.conv(xq, w0 + 3, ONE, ONE, True)
        h2y = self.store(h2[0], f"{name}.h2")
        b2 = self.conv(h2y, w0 + 4, THREE, ONE, False)
        pm = self.store(self.pool(xpool, THREE, ONE, f"{name}.b3a"), f"{name}.pm")
        b3 = self.conv(pm, w0 + 5, ONE, ONE, False)
        if self.audit is not None and x.requires_grad:
            convs = [r for r in self.audit[n0:] if r["kind"] == "conv" and r["tag"] in (f"unit{w0}", f"unit{w0 + 1}", f"unit{w0 + 3}")]
            self.audit.append(dict(kind="modin", tag=name, convs=convs, pool=recp))
        order = [b0, b2, b1, b3] if self.take("a_swap") else [b0, b1, b2, b3]
        return tuple(torch.cat([b[i] for b in order], 1) for i in range(3))


def reference(case, dtype=torch.float64, mode=0, wrong=None, audit=None, live=None, grads=None):
    """The plan slice in `dtype` on the CPU: dict(outs={endpoint: y}, dx=, dw={unit: grad}, applied=did the wrong variant find a
    site).  mode 0: fp32-operand; 1: bf16 operands and dz; 2 / 3: 1 plus bf16 storage of every activation and data gradient of
    the steps case.stored (and of x where case.x_half), as the class docstring of I3DFeaturesFunction states it: activations are
    kept as bf16 (pools choose among the rounded values), every stored data gradient is rounded once, a module's input gradient is
    bf16(bf16(fused 1x1 data gradient) + branch pool backward).  audit: a list that receives the records
    audit_failures() reads; live: a dict that receives the liveliness counts; grads: other upstream gradients than the case's."""
    R = _Run(case, dtype, mode, wrong, audit, live)
    if live is not None:
        live.update(pre_zero=0, pools=0, pool_ties=0, pad_ties=0, padded=0)
    x = case.x.detach().clone().to(dtype).requires_grad_(case.need_dx)
    grads = {e: g.to(dtype) for e, g in (grads or case.grads).items()}
    R.storing = mode >= 2 and case.x_half
    cur = R.store(x, "x")
    cur_pre = None              # the pre-activation of `cur` when it is a conv / module output
    outs, raws = {}, {}
    for si, step in enumerate(case.plan):
        kind, name = step[0], step[-1]
        consumed = si + 1 < len(case.plan)
        R.storing = mode >= 2 and case.stored[0] <= si < case.stored[1]
        if kind == "conv":
            y, pre, z = R.conv(cur, step[1], step[2], step[3], consumed)
        elif kind == "pool":
            y, pre, z = R.pool(cur, step[1], step[2], name), None, None
        else:
            xin = cur
            if cur_pre is not None and R.take("c_nomask"):
                xin = cur.detach() + (cur_pre - cur_pre.detach())
            y, pre, z = R.mixed(xin, step[1], step[2], name)
        y = R.store(y, name)
        if name in case.endpoints:
            outs[name] = y
            raws[name] = z
            if consumed and audit is not None and y.requires_grad:
                rec = dict(kind="part", g=None)
                audit.append(dict(kind="sum", tag=name, parts=[rec, dict(g=grads[name])]))
                y = _tap(y, rec)
        cur, cur_pre = y, pre
    heads = []
    for e in case.endpoints:
        if raws[e] is not None and R.take("f_rawadd"):
            heads.append(raws[e])
        else:
            heads.append(outs[e])
    inputs = ([x] if case.need_dx else []) + [R.w[u] for u in case.units]
    got = torch.autograd.grad(heads, inputs, [grads[e] for e in case.endpoints], allow_unused=True)
    got = [torch.zeros_like(t) if g is None else g for g, t in zip(got, inputs)]
    dx = got.pop(0) if case.need_dx else None
    if audit is not None:
        for u, g in zip(case.units, got):
            audit.append(dict(kind="stored", tag=f"dw{u}", t=g))
        if dx is not None:
            audit.append(dict(kind="stored", tag="dx", t=dx))
    return dict(outs={e: outs[e].detach() for e in case.endpoints}, dx=dx, dw=dict(zip(case.units, got)), applied=R.applied)


def compared(res):
    """name -> numpy array of everything the GPU test compares."""
    out = {f"out.{e}": t.numpy() for e, t in res["outs"].items()}
    if res["dx"] is not None:
        out["dx"] = res["dx"].numpy()
    out.update({f"dw{u}": g.numpy() for u, g in res["dw"].items()})
    return out


# ---------------------------------------------------------------------------------------------- the audit
def unit_exp(t):
    """The largest e such that every element of the float64 tensor t is an integer multiple of 2^e (None: t is all zero)."""
    a = t.detach().double().numpy().ravel()
    a = a[a != 0]
    if a.size == 0:
        return None
    m, e = np.frexp(a)
    M = np.ldexp(np.abs(m), 53).astype(np.int64)
    low = M & -M
    return int((e - 53 + np.frexp(low.astype(np.float64))[1] - 1).min())


def _fits(bound, exps):
    """sum |a||b| <= 2^24 u, u = 2^(sum of the operands' unit exponents)?  -> (ok, bits used)"""
    if bound == 0 or any(e is None for e in exps):
        return True, 0.0
    bits = math.log2(bound) - sum(exps)
    return bound <= math.ldexp(1.0, MANTISSA + sum(exps)), bits


def audit_failures(records):
    """([failures], most bits any accumulation uses).  Every accumulation's sum |a_i||b_i| against 2^24 u, and every stored tensor
    against fp32."""
    fails, worst = [], 0.0

    def check(tag, bound, exps):
        nonlocal worst
        ok, bits = _fits(float(bound), exps)
        worst = max(worst, bits)
        if not ok:
            fails.append((tag, round(bits, 2)))

    for r in records:
        if r["kind"] == "conv":
            ax, aw = r["x"].abs().double().requires_grad_(True), r["w"].abs().double().requires_grad_(True)
            az = F.conv3d(O._pad3(ax, r["k"], r["s"]), aw, None, stride=tuple(r["s"]))
            ux, uw = unit_exp(ax), unit_exp(aw)
            check(r["tag"] + ".fwd", az.detach().max(), [ux, uw])
            r["absdx"], r["udx"] = None, None
            if r["g"] is not None:
                g = r["g"].double()
                ug = unit_exp(g)
                adx, adw = torch.autograd.grad(az, [ax, aw], g.abs())
                check(r["tag"] + ".wgrad", adw.max(), [ux, ug])
                if r["dx"]:
                    check(r["tag"] + ".dgrad", adx.max(), [uw, ug])
                    r["absdx"], r["udx"] = adx, (None if ug is None or uw is None else ug + uw)
                if not torch.equal(g.float().double(), g):
                    fails.append((r["tag"] + ".dz not fp32", None))
        elif r["kind"] == "affine":
            z, sc, sh = r["z"].double(), r["sc"].double(), r["sh"].double()
            uz, us, uh = unit_exp(z), unit_exp(sc), unit_exp(sh)
            us_ = [e for e in (None if uz is None else uz + us, uh) if e is not None]
            check(r["tag"] + ".affine", (z.abs() * sc.abs() + sh.abs()).max(), [min(us_) if us_ else None])
        elif r["kind"] == "pool" and r["g"] is not None:
            g = r["g"].double()
            overlap = int(np.prod([-(-k // s) for k, s in zip(r["k"], r["s"])]))     # windows that can route into one element
            check(r["tag"] + ".poolbwd", g.abs().max() * overlap, [unit_exp(g)])
        elif r["kind"] == "modin":
            parts = [(c["absdx"], c["udx"]) for c in r["convs"] if c.get("absdx") is not None]
            if r["pool"] is not None and r["pool"]["g"] is not None:
                parts.append((r["pool"]["g"].double().abs(), unit_exp(r["pool"]["g"])))
            us = [u for _, u in parts if u is not None]
            if us:
                check(r["tag"] + ".input gradient", sum(p for p, _ in parts).max(), [min(us)])
        elif r["kind"] == "sum":
            gs = [p["g"].double() for p in r["parts"] if p["g"] is not None]
            us = [u for u in map(unit_exp, gs) if u is not None]
            if us:
                check(r["tag"] + ".endpoint sum", sum(g.abs() for g in gs).max(), [min(us)])
        elif r["kind"] == "stored":
            t = r["t"].double()
            if not torch.equal(t.float().double(), t):
                fails.append((r["tag"] + " not fp32", None))
    return fails, worst


# ---------------------------------------------------------------------------------------------- the cases
# Tuned on the CPU until audit_failures() is empty in every mode the case runs in (the audit derives the condition; these value
# ranges only have to meet it).  nnz = 24 non-zero weights per output channel keeps sum |x||w| near 24 max|x| whatever the fan-in;
# the unit shrinks by up to 2^-4 per layer, which is why no slice is more than two modules deep and the deep ones use fewer scales.
# label -> Case arguments; get_case() builds a case when a test first asks for it (importing this file builds nothing)
SLICES = {
    # Conv3d_1a on a (2,3,8,96,96) clip: the first-layer branch without dx (weight gradient on the main lane), and with dx
    "1a": dict(steps=["Conv3d_1a"], planes=(8, 96, 96), need_dx=False, seed=11),
    "1a.dx": dict(steps=["Conv3d_1a"], planes=(8, 96, 96), seed=12),
    "1a+2a": dict(steps=["Conv3d_1a", "MaxPool3d_2a"], planes=(8, 96, 96), need_dx=False, seed=13),
    "1a+2a.dx": dict(steps=["Conv3d_1a", "MaxPool3d_2a"], planes=(8, 96, 96), seed=14),
    # the (4,24,24) planes: a conv behind a conv (mask and scale in the data-gradient epilogue), a pool behind a conv (sign bits)
    "2b": dict(steps=["Conv3d_2b"], planes=(4, 24, 24), seed=21, gmax=300),
    "2b+2c": dict(steps=["Conv3d_2b", "Conv3d_2c"], planes=(4, 24, 24), seed=22),
    "2b+2c.nodx": dict(steps=["Conv3d_2b", "Conv3d_2c"], planes=(4, 24, 24), need_dx=False, seed=23),
    "2b+2c+3a": dict(steps=["Conv3d_2b", "Conv3d_2c", "MaxPool3d_3a"], planes=(4, 24, 24), seed=24),
    # the (4,12,12) planes: a module behind a pool (raw input, no mask), first, behind a module, in front of the 3x3x3 pool
    "3a+3b": dict(steps=["MaxPool3d_3a", "Mixed_3b"], planes=(4, 24, 24), seed=31),
    "3b": dict(steps=["Mixed_3b"], planes=(4, 12, 12), seed=32, gmax=9),
    "3b.nodx": dict(steps=["Mixed_3b"], planes=(4, 12, 12), need_dx=False, seed=33),
    "3b+3c": dict(steps=["Mixed_3b", "Mixed_3c"], planes=(4, 12, 12), seed=34, exps=(1, 2)),
    "3c+4a": dict(steps=["Mixed_3c", "MaxPool3d_4a"], planes=(4, 12, 12), seed=35),
    # the (4,6,6) planes; MaxPool3d_5a is the 2x2x2 pool and a pool that starts a plan (no sign bits)
    "4b": dict(steps=["Mixed_4b"], planes=(4, 6, 6), seed=41, gmax=9),
    "4f+5a+5b": dict(steps=["Mixed_4f", "MaxPool3d_5a", "Mixed_5b"], planes=(4, 6, 6), seed=42, exps=(1, 2)),
    "5a+5b": dict(steps=["MaxPool3d_5a", "Mixed_5b"], planes=(4, 6, 6), seed=43),
    "5c": dict(steps=["Mixed_5c"], planes=(2, 3, 3), seed=51, gmax=9),
    # odd planes and T = 3: the SAME padding is asymmetric
    "odd.2c": dict(steps=["Conv3d_2c"], planes=(3, 5, 7), seed=61),
    "odd.2c+3a": dict(steps=["Conv3d_2c", "MaxPool3d_3a"], planes=(3, 5, 7), seed=62),
    "odd.4a": dict(steps=["MaxPool3d_4a"], planes=(3, 5, 7), seed=63),
    "odd.3b": dict(steps=["Mixed_3b"], planes=(3, 5, 7), seed=64, gmax=9),
}
HANDOVER = {
    # two endpoints, the first also consumed downstream: the accumulate branch of masked_scale_copy
    "4f*+5a+5b*": dict(steps=["Mixed_4f", "MaxPool3d_5a", "Mixed_5b"], planes=(4, 6, 6), endpoints=["Mixed_4f", "Mixed_5b"], seed=71,
                       exps=(1, 2)),
    # an endpoint on a pool output together with a later one: the raw add_ branch and the clone
    "3c+4a*+4b*": dict(steps=["Mixed_3c", "MaxPool3d_4a", "Mixed_4b"], planes=(4, 12, 12), endpoints=["MaxPool3d_4a", "Mixed_4b"],
                       seed=72, exps=(1, 2)),
}
# gmax: the upstream gradients are integers up to 2; 9 where a single module shall hold a gradient operand dz of more than 8 bits
# (dh1, dh2: sums of some thirty such terms), 300 where a single convolution shall (dz = g * scale itself) -- so that the bf16
# rounding of dz in mode 1 is live in shallow slices too (wrong variant g)
# bf16 storage (ops.HALF_STORAGE + ops.HALF_CHAIN, mode 2): the single blocks of tests/test_bf16_layer_pin_gpu.py (BLOCKS) and its two
# pairs.  The 6x6 modules run at T = 8: at T = 4 _step_half_ok refuses them (the bf16-tensor kernels of the 1x1x1 layers want more
# positions), T = 8 is the smallest it accepts.  Behind Mixed_4f the region ends: MaxPool3d_5a + Mixed_5b take a bf16 x through the
# conversion seam and run on fp32 tensors, Mixed_5c never sees a bf16 tensor.
STORED = {
    "s.1a+2a": dict(steps=["Conv3d_1a", "MaxPool3d_2a"], planes=(8, 96, 96), need_dx=False, seed=81, x_half=False, xmax=31),
    "s.2b": dict(steps=["Conv3d_2b"], planes=(4, 24, 24), seed=82, gmax=300),
    "s.2c+3a": dict(steps=["Conv3d_2c", "MaxPool3d_3a"], planes=(4, 24, 24), seed=83, xmax=31),
    "s.3b": dict(steps=["Mixed_3b"], planes=(4, 12, 12), seed=84, gmax=9),
    "s.3c+4a": dict(steps=["Mixed_3c", "MaxPool3d_4a"], planes=(4, 12, 12), seed=85, gmax=9),
    "s.4b": dict(steps=["Mixed_4b"], planes=(8, 6, 6), seed=86, gmax=9),
    "s.4c": dict(steps=["Mixed_4c"], planes=(8, 6, 6), seed=87, gmax=9),
    "s.4d": dict(steps=["Mixed_4d"], planes=(8, 6, 6), seed=88, gmax=9),
    "s.4e": dict(steps=["Mixed_4e"], planes=(8, 6, 6), seed=89, gmax=9),
    "s.4f": dict(steps=["Mixed_4f"], planes=(8, 6, 6), seed=90, gmax=9),
    "s.5a+5b": dict(steps=["MaxPool3d_5a", "Mixed_5b"], planes=(4, 6, 6), seed=91, gmax=9, stored=(0, 0)),
    "s.5c": dict(steps=["Mixed_5c"], planes=(2, 3, 3), seed=92, gmax=9, x_half=False, stored=(0, 0)),
    "s.2b+2c+3a": dict(steps=["Conv3d_2b", "Conv3d_2c", "MaxPool3d_3a"], planes=(4, 24, 24), seed=93),
    "s.4e+4f": dict(steps=["Mixed_4e", "Mixed_4f"], planes=(8, 6, 6), seed=94, exps=(1, 2)),
}
# (xmax = 31 where a single layer is stored: its outputs shall need more than 8 bits, so that storing them is seen)
STORED_REGION = tuple(k for k in STORED if k not in ("s.5a+5b", "s.5c"))        # the slices that lie in the region as a whole
# bf16 storage of a layer's output in front of its strided pool WITHOUT the chain (mode 3: ops.HALF_ACT_DIRECT on, ops.HALF_CHAIN
# off): the pool reads the bf16 tensor as it is (pool_io1, no conversion seam).  The tape takes it for a layer BEHIND another one
# (Conv3d_2c behind Conv3d_2b: an fp32 gradient) and for the first layer without dx (Conv3d_1a: the gradient of its output is
# stored as bf16 too).  Conv3d_2c ALONE is neither -- HALF_ACT_DIRECT asks for a step in front, the first-layer form for a
# weight-gradient kernel that reads a bf16 dz, which only Conv3d_1a has -- so that slice stores nothing and equals mode 1.
DIRECT = {
    "d.2c+3a": dict(steps=["Conv3d_2c", "MaxPool3d_3a"], planes=(4, 24, 24), need_dx=False, seed=95, x_half=False, stored=(0, 0), xmax=31),
    "d.2b+2c+3a": dict(steps=["Conv3d_2b", "Conv3d_2c", "MaxPool3d_3a"], planes=(4, 24, 24), seed=96, x_half=False, stored=(1, 2)),
    "d.1a+2a": dict(steps=["Conv3d_1a", "MaxPool3d_2a"], planes=(8, 96, 96), need_dx=False, seed=97, x_half=False, stored=(0, 1), xmax=31),
}
HANDOVER_PAIRS = tuple(HANDOVER)
# the trunk cut of extract_features (split_backward) by hand: the same slice with its last endpoint alone
HANDOVER["3c+4a+4b"] = dict(steps=["Mixed_3c", "MaxPool3d_4a", "Mixed_4b"], planes=(4, 12, 12), seed=73, exps=(1, 2))
FP32_STORED = tuple(SLICES) + tuple(HANDOVER)       # run in modes 0 and 1 on fp32 tensors
SPECS = dict(SLICES, **HANDOVER, **STORED, **DIRECT)
RUNS = [(k, m) for k in FP32_STORED for m in (0, 1)] + [(k, 2) for k in STORED] + [(k, 3) for k in DIRECT]
# liveliness exceptions, with their reasons.  The only padded pool of this slice (Mixed_5b's branch pool) reads maxima of eight
# integers from [-3, 3]: a border window without a positive one does not occur, so nothing ties with the padding's 0
NO_PAD_TIE = ("5a+5b", "s.5a+5b")


def handover_grads(case, kind):
    """Other upstream gradients of a two-endpoint case: "only0" / "only1" -- the earlier / the later endpoint alone receives a
    non-zero one; "flat0" / "flat1" -- the earlier / the later one's is constant over the planes (one number per sample and
    channel: what a stride-0 expanded view can hold)."""
    which = case.endpoints[int(kind[-1])]
    if kind.startswith("flat"):
        return {e: (g[:, :, :1, :1, :1].expand_as(g).contiguous() if e == which else g) for e, g in case.grads.items()}
    return {e: (g if e == which else torch.zeros_like(g)) for e, g in case.grads.items()}


def min_nonzero(case, key):
    """The least non-zero share of a compared tensor: MIN_NONZERO, except for the input gradient of a slice that BEGINS with a
    strided pool -- a window routes its gradient to one element, so at most one element in prod(stride) can be non-zero."""
    if key == "dx" and case.plan[0][0] == "pool":
        return MIN_NONZERO / float(np.prod(case.plan[0][2]))
    return MIN_NONZERO
_BUILT = {}


def get_case(label):
    if label not in _BUILT:
        _BUILT[label] = Case(label, **SPECS[label])
    return _BUILT[label]
