"""An ANCHORED high-precision reference of CoarsePyramid.forward (AFSD/thumos14/BDNet.py:295-432, anet/BDNet.py:271-391),
shared by tests/test_pyramid_tape_ref_cpu.py and tests/test_pyramid_tape_gpu.py.  Test infrastructure: plain torch on the
CPU, per level and not packed, op for op the restatement of oracle/afsd_oracle.py::coarse_pyramid -- in a dtype of the
caller's choice and with the discrete decisions of ANOTHER run handed in.

Why anchored.  A float64 run of the detection half takes its own discrete decisions -- the sign of every ReLU input, the
winner of every BoundaryMaxPooling window, the rounded proposal windows -- and a few dozen of them differ from any fp32
run; each one moves whole weight rows, so an fp32 gradient sits 4e-3 (of the tensor's maximum) from the plain float64 one
and no elementwise check is possible.  The anchor is the forward state of the run under test:

  blocks    {conv weight key: [output per level]} of every Conv + GroupNorm + ReLU block.  The reference computes
            u = GroupNorm(conv(x)) in its own precision from its own input, masks it with the ANCHOR's sign,
            y = u * (y_dev > 0), and goes on with y + (y_dev - y).detach(): the value downstream is the anchor's, the
            gradient flows through the reference's arithmetic, the ReLU decision is the anchor's.  (`_Anchored` returns
            y_dev itself -- what that expression gives wherever the subtraction is exact -- so that the pools below see the
            anchor's values to the bit.)
  windows   (segments, frame_segments) (B, N, 4), the proposal windows of all levels side by side.
  merged    optional: level 0 after the top-down merge (an fp32 sum of two anchored maps on the device).

BoundaryMaxPooling acts on anchored maps, so winners and pooled values are the anchor's exactly; `bmp` states the rule of
boundary_max_pooling_kernel.cu:33-40 (as csrc/bmp.hip does) in any dtype.  Heads, ScaleExp, the fpn-stride factor and the
Dirichlet uncertainty are smooth and stay unanchored.  Under `O.operand_rounding("bf16")` both operands of every
convolution the device runs on the bf16 MFMA are rounded to bf16 before an exact product (the inputs are anchored: fp32
values, so the rounding is the device's).
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import afsd_oracle as O
from oracle import arch

Q = "coarse_pyramid_detection"
WIDE_HEAD = 21          # ops.HC_MAX_ROWS: heads up to this many rows are exact fp32 FMA kernels, wider ones take the GEMM path
M = 10.0                # the standing margin for "an independent draw with another summation order" (test_model_gpu.py:118-125)
FLOOR = 2.0 ** -23

COARSE = ("loc", "conf", "act", "unct")
REFINED = ("prop_loc", "prop_conf", "center", "prop_act", "prop_unct")
BOUNDARY = ("start", "end", "start_loc_prop", "end_loc_prop", "start_conf_prop", "end_conf_prop")
FRAME = ("start", "end")
OUTPUTS = COARSE + REFINED + BOUNDARY
SUBSETS = dict(all=OUTPUTS, coarse=COARSE, refined=REFINED, boundary=BOUNDARY, frame=FRAME)
SSL_OUTPUTS = ("frame", "loc_lr", "conf_lr")

conv1d = F.conv1d       # the 1-D convolution every block and head goes through (a stand-in device swaps it, see permuted_conv1d)


def permuted_conv1d(seed=7):
    """A 1-D convolution that sums a PERMUTED K in two halves: same mathematics, another summation order -- an fp32 run
    through it is the CPU stand-in for a device."""
    perms = {}

    def conv(x, w, b=None, stride=1):
        C = w.shape[1]
        if C not in perms:
            perms[C] = torch.from_numpy(np.random.RandomState(seed + C).permutation(C))
        p, h = perms[C], C // 2
        return F.conv1d(x[:, p[:h]], w[:, p[:h]], None, stride=stride) + F.conv1d(x[:, p[h:]], w[:, p[h:]], b, stride=stride)
    return conv


class swap_conv1d:
    def __init__(self, fn):
        self.fn = fn

    def __enter__(self):
        global conv1d
        self.old, conv1d = conv1d, self.fn

    def __exit__(self, *a):
        global conv1d
        conv1d = self.old


# ----------------------------------------------------------------------------------------------------------- pieces
def _r(t):
    """O._r in any float dtype: bf16 operand rounding with a pass-through gradient."""
    if O._ROUND == "bf16":
        return O._RoundOperand.apply(t) if t.requires_grad else t.to(torch.bfloat16).to(t.dtype)
    return t


class _Anchored(torch.autograd.Function):
    """y = u * (y_dev > 0); y + (y_dev - y).detach() -- with the value y_dev to the bit."""

    @staticmethod
    def forward(ctx, u, y_dev):
        ctx.save_for_backward(y_dev > 0)
        return y_dev.clone()

    @staticmethod
    def backward(ctx, g):
        (pos,) = ctx.saved_tensors
        return torch.where(pos, g, torch.zeros_like(g)), None


def _act(u, name, level, anchor, record):
    if anchor is None:
        y = F.relu(u)
    else:
        y_dev = anchor["blocks"][name][level].to(u.dtype)
        assert y_dev.shape == u.shape, (name, level, tuple(y_dev.shape), tuple(u.shape))
        y = _Anchored.apply(u, y_dev)
    if record is not None:
        record["blocks"].setdefault(name, {})[level] = y.detach().clone()
    return y


def unit1d(x, w, b, stride=1, exact=False):
    f, bk = O.same_pad(x.shape[2], w.shape[2], stride)
    if not exact:
        x, w = _r(x), _r(w)
    return conv1d(F.pad(x, [f, bk]), w, b, stride=stride)


def gn(x, gamma, beta):
    return F.group_norm(x, 32, gamma, beta, 1e-5)


def block_pre(P, prefix, x, stride=1, conv_idx=0, gn_idx=1):
    """u = GroupNorm(conv(x)) of a Unit1D block (before the ReLU) and the block's name."""
    name = f"{prefix}.{conv_idx}.conv1d.weight"
    u = unit1d(x, P[name], P[f"{prefix}.{conv_idx}.conv1d.bias"], stride)
    return gn(u, P[f"{prefix}.{gn_idx}.weight"], P[f"{prefix}.{gn_idx}.bias"]), name


def proj_pre(P, i, f):
    """u of a projection block: Unit3D 'spatial_valid' (temporal k = 1) + GroupNorm (BDNet.py:129-155)."""
    name = f"{Q}.pyramids.{i}.0.conv3d.weight"
    u = F.conv3d(_r(f), _r(P[name]), P[f"{Q}.pyramids.{i}.0.conv3d.bias"]).squeeze(-1).squeeze(-1)
    return gn(u, P[f"{Q}.pyramids.{i}.1.weight"], P[f"{Q}.pyramids.{i}.1.bias"]), name


def bmp_index(x, seg, chunk=32):
    """Winner positions (B, C, N) of BoundaryMaxPooling, boundary_max_pooling_kernel.cu:33-40: window bounds truncated and
    clamped to [0, T-1]; the scan starts at l and only a strictly greater value replaces the running maximum (the first
    maximum wins); an inverted window gives x[l]; the first half of the channels reads columns 0, 1, the second 2, 3."""
    B, C, T = x.shape
    N = seg.shape[1]
    assert seg.shape[0] == B and seg.shape[2] == 4 and C % 2 == 0
    half = C // 2
    idx = torch.empty((B, C, N), dtype=torch.int64)
    pos = torch.arange(T)
    with torch.no_grad():
        xd = x.detach()
        for h in range(2):
            l = seg[:, :, 2 * h].double().trunc().clamp(0, T - 1).long()[:, None, :, None]          # (B,1,N,1)
            r = seg[:, :, 2 * h + 1].double().trunc().clamp(0, T - 1).long()[:, None, :, None]
            inwin = ((pos >= l) & (pos <= r)) | (pos == l)                                          # (B,1,N,T)
            for c0 in range(h * half, (h + 1) * half, chunk):
                c1 = min(c0 + chunk, (h + 1) * half)
                v = xd[:, c0:c1, None, :].expand(B, c1 - c0, N, T)
                best = v.masked_fill(~inwin, -float("inf")).amax(-1, keepdim=True)
                hit = inwin & (v == best)
                idx[:, c0:c1] = torch.where(hit, T - pos, torch.zeros_like(pos)).argmax(-1)        # the lowest hit: unique maximum
    return idx


def bmp(x, seg, idx=None):
    """BoundaryMaxPooling in x's dtype; the gradient goes to the winner (contributions added per row)."""
    return x.gather(2, bmp_index(x, seg) if idx is None else idx)


def _head(P, name, x):
    w = P[f"{Q}.{name}.conv1d.weight"]
    return unit1d(x, w, P[f"{Q}.{name}.conv1d.bias"], exact=w.shape[0] <= WIDE_HEAD)


def params(params_np, dtype):
    """The pyramid's parameters of a numpy state dict as leaves of `dtype`."""
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(dtype).requires_grad_(True)
            for k, v in params_np.items() if k.startswith(Q + ".")}


# ----------------------------------------------------------------------------------------------------------- forward
def pyramid(P, f4, f5, cfg=arch.THUMOS, anchor=None, ssl=False, record=None):
    """CoarsePyramid.forward with os_head and the Dirichlet uncertainty maps -> dict of outputs (OUTPUTS; with ssl the three
    maps SSL_OUTPUTS, channel-major).  P, f4, f5 share one dtype; f4 is unused in the one-projection layout.
    anchor: see the module docstring; record: a dict that receives this run's own anchor."""
    if record is not None:
        record["blocks"] = {}
    frame_num = cfg["frame_num"]
    strides = cfg.get("fpn_strides")
    if cfg.get("two_projections", True):
        u0, n0 = proj_pre(P, 0, f4)
        x0 = _act(u0, n0, 0, anchor, record)
        u1, n1 = proj_pre(P, 1, f5)
        x1 = _act(u1, n1, 0, anchor, record)
        x0 = x0 + F.interpolate(x1, x0.shape[2:], mode="nearest")
        if anchor is not None and anchor.get("merged") is not None:
            x0 = x0 + (anchor["merged"].to(x0.dtype) - x0).detach()
        if record is not None:
            record["merged"] = x0.detach().clone()
        feats = [x0, x1]
        x = x1
    else:
        u, n = proj_pre(P, 0, f5)
        x = _act(u, n, 0, anchor, record)
        feats = [x]
    for i in range(len(feats), cfg["layer_num"]):
        u, n = block_pre(P, f"{Q}.pyramids.{i}", x, stride=2)
        x = _act(u, n, 0, anchor, record)
        feats.append(x)
    ff = F.interpolate(feats[0].unsqueeze(-1), [frame_num, 1]).squeeze(-1)
    for ci in (0, 3, 6):
        u, n = block_pre(P, f"{Q}.deconv", ff, 1, ci, ci + 1)
        ff = _act(u, n, 0, anchor, record)
    tr = lambda y: y.permute(0, 2, 1).contiguous()

    def block(prefix, x, i):
        u, n = block_pre(P, prefix, x)
        return _act(u, n, i, anchor, record)
    if ssl:         # the triplet branch: level 0 only (BDNet.py:392-398)
        lf, cf = feats[0], feats[0]
        for j in range(2):
            lf = block(f"{Q}.loc_tower.{j}", lf, 0)
            cf = block(f"{Q}.conf_tower.{j}", cf, 0)
        return {"frame": ff, "loc_lr": block(f"{Q}.loc_proposal_branch.lr_conv", lf, 0),
                "conf_lr": block(f"{Q}.conf_proposal_branch.lr_conv", cf, 0)}
    half = ff.shape[1] // 2
    out = {"start": tr(ff[:, :half]), "end": tr(ff[:, half:])}
    locs, confs, acts, plocs, pconfs, pacts, ctrs = [], [], [], [], [], [], []
    segs, fsegs, off = [], [], 0
    for i, feat in enumerate(feats):
        lf, cf = feat, feat
        for j in range(2):
            lf = block(f"{Q}.loc_tower.{j}", lf, i)
            cf = block(f"{Q}.conf_tower.{j}", cf, i)
        loc = tr(torch.exp(_head(P, "loc_head", lf) * P[f"{Q}.loc_heads.{i}.scale"]))
        if strides:
            loc = loc * strides[i]
        locs.append(loc)
        confs.append(tr(_head(P, "conf_head", cf)))
        acts.append(tr(_head(P, "actionness_head", cf)))
        t = feat.shape[2]
        if anchor is None:
            seg, fseg = O.proposal_windows(loc.detach().float(), t, frame_num)
        else:
            seg, fseg = (w[:, off:off + t] for w in anchor["windows"])
        off += t
        segs.append(seg)
        fsegs.append(fseg)
        fidx = bmp_index(ff, fseg)          # (the reference pools the frame-level map once per branch: same winners)
        props = []
        for br, x in (("loc_proposal_branch", lf), ("conf_proposal_branch", cf)):
            short = block(f"{Q}.{br}.cur_point_conv", x, i)
            lr = block(f"{Q}.{br}.lr_conv", x, i)
            pooled = bmp(lr, seg)
            roi = block(f"{Q}.{br}.roi_conv", bmp(ff, fseg, fidx), i)
            props.append((block(f"{Q}.{br}.proposal_conv", torch.cat([roi, pooled, short], 1), i), lr))
            if record is not None:
                record.setdefault("pooled", {}).setdefault(br, {})[i] = pooled.detach().clone()
        (lp, lp_lr), (cp, cp_lr) = props
        if i == 0:
            nd = lp_lr.shape[1] // 2
            out["start_loc_prop"], out["end_loc_prop"] = tr(lp_lr[:, :nd]), tr(lp_lr[:, nd:])
            out["start_conf_prop"], out["end_conf_prop"] = tr(cp_lr[:, :nd]), tr(cp_lr[:, nd:])
        plocs.append(tr(_head(P, "prop_loc_head", lp)))
        pconfs.append(tr(_head(P, "prop_conf_head", cp)))
        pacts.append(tr(_head(P, "prop_actionness_head", cp)))
        ctrs.append(tr(_head(P, "center_head", lp)))
    out.update(loc=torch.cat(locs, 1), conf=torch.cat(confs, 1), act=torch.cat(acts, 1), prop_loc=torch.cat(plocs, 1),
               prop_conf=torch.cat(pconfs, 1), prop_act=torch.cat(pacts, 1), center=torch.cat(ctrs, 1))
    out["unct"] = O.dirichlet_uncertainty(out["conf"])
    out["prop_unct"] = O.dirichlet_uncertainty(out["prop_conf"])
    if record is not None:
        record["windows"] = (torch.cat(segs, 1), torch.cat(fsegs, 1))
        record["blocks"] = {n: [d[l] for l in sorted(d)] for n, d in record["blocks"].items()}
    return out


def ref_block(P, name, x, levels=None, stride=1):
    """relu(GroupNorm(conv(x))) of the block whose conv weight is `name`, applied to that block's own (device) input: a
    (B, C, T, H, W) endpoint for a projection, else a (B, C, T) map -- with `levels` a packed one, convolved and normalised
    level by level."""
    if name.endswith("conv3d.weight"):
        i = int(name.split(".")[2])
        return F.relu(proj_pre(P, i, x)[0])
    prefix, ci = name[:-len(".conv1d.weight")].rsplit(".", 1)
    ci = int(ci)
    lev = levels if levels is not None else (0, x.shape[2])
    return torch.cat([F.relu(block_pre(P, prefix, x[:, :, lev[l]:lev[l + 1]], stride, ci, ci + 1)[0])
                      for l in range(len(lev) - 1)], 2)


# ----------------------------------------------------------------------------------------------------------- runs
def endpoints(seed, batch, cfg=arch.THUMOS):
    """Non-negative endpoint maps (a ReLU's output: half the entries zero), activations O(1)."""
    rs = np.random.RandomState(seed)
    t0 = cfg["feat_t"]
    if cfg.get("two_projections", True):
        f4 = np.maximum(rs.standard_normal((batch, cfg["feat_channels"][0], t0, 6, 6)), 0).astype(np.float32)
        f5 = np.maximum(rs.standard_normal((batch, cfg["feat_channels"][1], t0 // 2, 3, 3)), 0).astype(np.float32)
        return torch.from_numpy(f4), torch.from_numpy(f5)
    f5 = np.maximum(rs.standard_normal((batch, cfg["feat_channels"][0], t0, 3, 3)), 0).astype(np.float32)
    return None, torch.from_numpy(f5)


def cotangents(seed, out, names):
    """Fixed random cotangents {name: fp32 tensor} for the outputs `names` of `out` (shapes only are read)."""
    rs = np.random.RandomState(seed)
    return {k: torch.from_numpy(rs.standard_normal(tuple(out[k].shape)).astype(np.float32)) for k in names}


class Run:
    """One graph of the reference: outputs, and the gradients of sum(out * cotangent) over a subset of the outputs w.r.t.
    every parameter and both endpoints (retain_graph: one graph serves all subsets)."""

    def __init__(self, params_np, f4, f5, cfg, dtype, anchor=None, ssl=False, record=None):
        self.P = params(params_np, dtype)
        self.f4 = None if f4 is None else f4.detach().to(dtype, copy=True).requires_grad_(True)     # (leaves of its own)
        self.f5 = f5.detach().to(dtype, copy=True).requires_grad_(True)
        self.out = pyramid(self.P, self.f4, self.f5, cfg, anchor, ssl, record)
        self.names = sorted(self.P) + (["input.f4"] if self.f4 is not None else []) + ["input.f5"]

    def grads(self, cot, subset):
        """{name: gradient or None (no path from the subset)}."""
        leaves = [self.P[n] for n in sorted(self.P)] + ([self.f4] if self.f4 is not None else []) + [self.f5]
        cost = sum((self.out[k] * cot[k].to(self.out[k].dtype)).sum() for k in subset)
        gs = torch.autograd.grad(cost, leaves, retain_graph=True, allow_unused=True)
        return dict(zip(self.names, gs))


class Reference:
    """The anchored reference of one configuration: the float64 run and the float32 evaluations that measure E32 on the
    same anchor (the plain one, and one per DRAW_SEEDS with another summation order, see `distance`)."""

    def __init__(self, params_np, f4, f5, cfg, anchor, ssl=False):
        self.anchor = anchor
        self.r64 = Run(params_np, f4, f5, cfg, torch.float64, anchor, ssl)
        self.r32 = Run(params_np, f4, f5, cfg, torch.float32, anchor, ssl)
        self.more = []
        for seed in DRAW_SEEDS:
            with swap_conv1d(permuted_conv1d(seed)):
                self.more.append(Run(params_np, f4, f5, cfg, torch.float32, anchor, ssl))
        self._grads = {}

    def outputs(self):
        """(float64 outputs, E32 per output)"""
        return self.r64.out, distance(self.r64.out, self.r32.out, [m.out for m in self.more])

    def grads(self, cot, subset):
        """(float64 gradients, E32 per gradient) of the cotangents `cot` on the outputs `subset`, computed once."""
        key = tuple(subset)
        if key not in self._grads:
            g64 = self.r64.grads(cot, subset)
            self._grads[key] = (g64, distance(g64, self.r32.grads(cot, subset), [m.grads(cot, subset) for m in self.more]))
        return self._grads[key]


# ----------------------------------------------------------------------------------------------------------- tolerance
def family(name):
    if name.startswith("input.") or name in OUTPUTS or name in SSL_OUTPUTS:
        return name
    n = name[len(Q) + 1:]
    head = n.split(".")[0]
    if head in ("pyramids", "deconv", "loc_heads"):
        return head
    if head.endswith("_tower"):
        return "towers"
    if head.endswith("_proposal_branch"):
        return "branches." + n.split(".")[1]
    return "heads"


TINY = 16               # a tensor with fewer elements (the ScaleExp scales, the 1- and 2-row heads' biases) takes E32 over all draws
DRAW_SEEDS = (101, 202)


def distance(ref64, ref32, more=()):
    """{name: E32 = max|ref32 - ref64|, or None where the reference has no gradient}: both runs on the same anchor.
    `more`: further fp32 evaluations of the anchored reference with other summation orders (`permuted_conv1d`).  They count
    only for tensors of fewer than TINY elements: E32 of a wide tensor is the largest of many draws and stable, E32 of a
    scalar is ONE draw of the fp32 error and lies below a tenth of its spread with probability 0.08 -- with a dozen such
    tensors in five cotangent sets the rule would fail by chance.  The largest of three draws does so with 5e-4."""
    out = {}
    for n, r64 in ref64.items():
        assert (r64 is None) == (ref32[n] is None), n
        if r64 is None:
            out[n] = None
            continue
        draws = [ref32] + (list(more) if r64.numel() < TINY else [])
        out[n] = max(float((d[n].detach().double() - r64.detach().double()).abs().max()) for d in draws)
    return out


def ratios(got, ref64, e32):
    """Per tensor: max|got - ref64| / max(E32, 2^-23 max|ref64|): the yardstick is the reference's own fp32 distance on
    the same anchor (`distance`), never the code under test.  None stands for a zero gradient; a tensor the reference has as
    exactly zero must be exactly zero (ratio 0 or inf)."""
    out = {}
    for n, r64 in ref64.items():
        g = got.get(n)
        if r64 is None:
            out[n] = 0.0 if (g is None or not bool(g.detach().ne(0).any())) else float("inf")
            continue
        r64 = r64.detach().double().cpu()
        g = torch.zeros_like(r64) if g is None else g.detach().double().cpu()
        assert g.shape == r64.shape, (n, tuple(g.shape), tuple(r64.shape))
        bound = max(e32[n], FLOOR * float(r64.abs().max()))
        err = float((g - r64).abs().max())
        out[n] = err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))
        if not np.isfinite(err):
            out[n] = float("inf")
    return out


def worst_by_family(rat):
    fam = {}
    for n, v in rat.items():
        f = family(n)
        if v >= fam.get(f, (-1.0, ""))[0]:
            fam[f] = (v, n)
    return fam


def check(got, ref64, e32, what, m=M):
    """Assert the tolerance rule on every tensor of ref64; prints the worst ratio per family.  -> {family: (ratio, name)}"""
    rat = ratios(got, ref64, e32)
    fam = worst_by_family(rat)
    print(f"[{what}] worst ratio per family: " + ", ".join(f"{f} {v:.3g}" for f, (v, _) in sorted(fam.items())))
    bad = sorted(((v, n) for n, v in rat.items() if not v <= m), reverse=True)
    assert not bad, f"{what}: {len(bad)} of {len(rat)} tensors beyond {m} x the reference's fp32 distance: {bad[:8]}"
    return fam
