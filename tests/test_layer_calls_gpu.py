"""GPU: every max-pool, GroupNorm and glue call the model makes (tests/golden/layer_calls.npz: a THUMOS14 training step at
b = 8 and b = 1, the same b = 8 step with fp32 pool tensors, an ActivityNet step at b = 2, an inference batch), replayed
through the C ABI with the recorded geometry, strides, io bits, flags and pointer alignment, and compared with the float64 /
exact reference (oracle/layer_ref.py) on EVERY element.

Options are the table defaults of options.h.  Pool rows run with at most two samples (the batch only adds workgroup rows).
Variants per recorded row reach the other kernels the same call can take: OTAL_POOL_NO133 / OTAL_POOL_NOROWS, nonneg off for the ordered-key rows, a winner-byte buffer at an odd address (no 8-column
kernel), the bf16 -> fp32 twin of every bf16 pool row, the io = 1 (bf16 x / dx only) form of the (1,3,3)/(1,2,2) rows,
misaligned fp32 branch pools (the cell-per-thread kernels), non-negative inputs for the bf16 (1,3,3)/(1,2,2) rows (the
ordered-key kernel; the model does not promise nonneg today), and a contiguous twin of every sliced GroupNorm dy.  EXTRA
holds what the model never runs: the run-time-shaped pools and the four compile-time ones, with and without LDS staging,
GroupNorm with T % 4 != 0, short and many levels, keep_dx off, three unequal terms, the pair form.

Per launch: the outputs start as a pattern no kernel writes (NaN or random when accumulating); every element must be
written, everything else in the buffers (other channels, slack, a guard tail) keeps its sentinel bits; forward values,
winner bytes, sign bits and conversions match exactly; every summed result meets
    |got - ref| <= C * 2^-24 * f(K) * e + r * |ref|
with ONE constant C per family (C_POOL, C_GN, C_GLUE) and r the output's storage rounding; otal_layer_last_kernel() names
the kernel, and for a pool it is the kernel (or the refusal) pool_choose() answers for the same call on the CPU
(opental_amd/csrc/pool_select.h through tests/cpu_pool_select.cpp).  A GroupNorm backward's ReLU mask is the LIBRARY forward's y > 0, so a forward / backward disagreement is a
full-size error.  The last item checks that every kernel name in POOL_KERNELS / GN_PATHS was reached."""
import contextlib
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import pool_select_harness as PS
from oracle import layer_ref as R

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
Z = np.load(os.path.join(HERE, "golden", "layer_calls.npz"))
NROWS = len(Z["entry"])
U = 2.0 ** -24
R_BF16, R_FP32 = 2.0 ** -8, 2.0 ** -24
C_POOL = 1.0        # f(K) = K: the pool backward adds at most 27 terms per stage, then scale and old (worst case, no sqrt)
C_GN = 4.0          # f(K) = sqrt(K): blocked fp32 sums over a group level of K elements
C_GLUE = 1.0        # f(K) = K
GUARD = 256
SENT32, SENT16, SENT8 = 0x7F7FBEEF, 0x7F5B, 0xEE
E_SHAPE, E_UNSUPPORTED = -2, -7
OPTIONS = [(n, int(v)) for n, v in re.findall(r'\{"(OTAL_\w+)",\s*(\d+)\}',
                                                open(os.path.join(REPO, "opental_amd", "csrc", "options.h")).read())]
POOL_KERNELS = (
    "maxpool133_s2_w8_nn_fwd", "maxpool133_s2_w8_fwd", "maxpoolk33_s2_fwd<1,bf16,bf16>", "maxpoolk33_s2_fwd<3,bf16,bf16>",
    "maxpoolk33_s2_fwd<1,bf16,f32>", "maxpoolk33_s2_fwd<1,f32,f32>", "maxpoolk33_s2_fwd<3,f32,f32>",
    "maxpool333_rows_fwd<12,bf16>", "maxpool333_rows_fwd<6,bf16>", "maxpool333_rows_fwd<12,f32>", "maxpool333_rows_fwd<6,f32>",
    "maxpool333_sep_fwd<12>", "maxpool333_sep_fwd<6>", "maxpool333_sep_fwd<3>",
    "maxpool3d_fwd<133/122>", "maxpool3d_fwd<333/111>", "maxpool3d_fwd<333/222>", "maxpool3d_fwd<222/222>", "maxpool3d_fwd<generic>",
    "maxpool3d_fwd_lds<333/111>", "maxpool3d_fwd_lds<generic>",
    "maxpool133_s2_w8_bwd", "maxpoolk33_s2_bwd<1,bf16,bf16>", "maxpool333_s2_w12_bwd", "maxpoolk33_s2_bwd<3,bf16,bf16>",
    "maxpoolk33_s2_bwd<1,bf16,f32>", "maxpoolk33_s2_bwd<1,f32,f32>", "maxpoolk33_s2_bwd<3,f32,f32>",
    "maxpool333_rows_bwd<12,bf16>", "maxpool333_rows_bwd<6,bf16>", "maxpool333_rows_bwd<12,f32>", "maxpool333_rows_bwd<6,f32>",
    "maxpool333_sep_bwd<12,v4>", "maxpool333_sep_bwd<6,v4>", "maxpool333_sep_bwd<12>", "maxpool333_sep_bwd<6>",
    "maxpool333_sep_bwd<3>") + tuple(f"maxpool3d_bwd{s}<{k}>" for s in ("", "_lds")
                                     for k in ("133/122", "333/111", "333/222", "222/222", "generic"))
GN_PATHS = ("gn_relu_fwd<single>", "gn_relu_fwd<pair>", "gn_relu_bwd<single,keep_dx,terms=0>",
            "gn_relu_bwd<single,no_keep_dx,terms=0>", "gn_relu_bwd<pair,keep_dx,terms=0>", "gn_relu_bwd<single,keep_dx,terms=1>",
            "gn_relu_bwd<single,keep_dx,terms=2>", "gn_relu_bwd<single,keep_dx,terms=3>", "gn_relu_bwd<single,no_keep_dx,terms=3>")
REACHED = set()
WORST = {}
EDGE = {"n": 0}


def fam(i):
    return R.FAMILY[str(Z["entry"][i])]


def row(i):
    return R.unpack(fam(i), Z["ints"][i]), [int(v) for v in Z["addr16"][i]]


# ------------------------------------------------------------------------------------------------ items
def pool_geom(thw, k, s, B=1, C=2):
    pads, outs = [], []
    for size, kk, ss in zip(thw, k, s):
        total = max((kk - ss) if size % ss == 0 else (kk - size % ss), 0)
        pads.append(total // 2)
        outs.append((size + total - kk) // ss + 1)
    return [B, C, *thw, *outs, *k, *s, *pads]


def pool_extra():
    """(name, family, ints, addr16): pool instantiations the model never reaches."""
    out = []
    shapes = [("133-odd", (3, 7, 9), (1, 3, 3), (1, 2, 2)), ("133-big", (2, 201, 203), (1, 3, 3), (1, 2, 2)),
              ("333s1-5x7", (6, 5, 7), (3, 3, 3), (1, 1, 1)), ("333s1-big", (3, 120, 121), (3, 3, 3), (1, 1, 1)),
              ("333s2-odd", (5, 7, 9), (3, 3, 3), (2, 2, 2)), ("333s2-big", (3, 201, 203), (3, 3, 3), (2, 2, 2)),
              ("222", (4, 5, 7), (2, 2, 2), (2, 2, 2)), ("222-big", (2, 201, 203), (2, 2, 2), (2, 2, 2)),
              ("gen-231", (5, 6, 7), (2, 3, 1), (1, 2, 1)), ("gen-222s1", (4, 5, 6), (2, 2, 2), (1, 1, 1)),
              ("gen-222s1-big", (3, 120, 122), (2, 2, 2), (1, 1, 1)), ("sep3", (7, 3, 3), (3, 3, 3), (1, 1, 1)),
              ("333s2-w8-bf16", (4, 6, 8), (3, 3, 3), (2, 2, 2))]
    for name, thw, k, s in shapes:
        g = pool_geom(thw, k, s)
        P, Po = thw[0] * thw[1] * thw[2], g[5] * g[6] * g[7]
        st = [2 * P, P, 2 * Po, Po]
        io = 3 if name.endswith("bf16") else 0
        out.append((name, "pool_fwd", g + st + [io, 0, 0], [0] * 5))
        for acc, mask in ((0, 0), (1, 1)):
            if io and (acc or mask):
                continue
            out.append((f"{name}-acc{acc}", "pool_bwd", g + st + [io, acc, mask, mask or io, io], [0] * 5))
    return out


def gn_extra():
    """(name, family, ints, eps): GroupNorm paths the model never reaches."""
    def fwd(B, C, T, G, lev=None, pair=0):
        nl = len(lev) - 1 if lev else 1
        return [B, C, T, G, 1, pair, 0, 0, nl] + ((list(lev) if lev else []) + [0] * 9)[:9]

    def bwd(B, C, T, G, lev=None, pair=0, terms=()):
        nl = len(lev) - 1 if lev else 1
        t = [v for tt in terms for v in tt] + [0] * (9 - 3 * len(terms))
        return [B, C, T, G, 1, pair, nl] + ((list(lev) if lev else []) + [0] * 9)[:9] + [0, len(terms)] + t
    lev8 = [0, 64, 96, 112, 120, 124, 126, 127, 129]
    return [("T37", "gn_fwd", fwd(2, 64, 37, 32)), ("T37", "gn_bwd", bwd(2, 64, 37, 32)),
            ("short-levels", "gn_fwd", fwd(2, 64, 70, 32, [0, 48, 62, 66, 69, 70])),
            ("short-levels", "gn_bwd", bwd(2, 64, 70, 32, [0, 48, 62, 66, 69, 70])),
            ("nlev8", "gn_fwd", fwd(1, 64, 129, 32, lev8)), ("nlev8", "gn_bwd", bwd(1, 64, 129, 32, lev8)),
            ("no-keep-dx", "gn_fwd", fwd(2, 64, 500, 2)), ("no-keep-dx", "gn_bwd", bwd(2, 64, 500, 2)),
            ("no-keep-dx-3terms", "gn_bwd", bwd(1, 64, 500, 2, terms=((64 * 500, 500, 500), (64 * 300, 300, 300), (64 * 512, 512, 17)))),
            ("3terms-unequal", "gn_bwd", bwd(2, 64, 37, 32, [0, 24, 37], terms=((64 * 37, 37, 37), (64 * 40, 40, 24), (128 * 37, 37, 5)))),
            ("1term", "gn_bwd", bwd(2, 64, 37, 32, terms=((96 * 40, 40, 37),))),
            ("pair", "gn_fwd", fwd(2, 64, 40, 32, pair=1)), ("pair", "gn_bwd", bwd(2, 64, 40, 32, pair=1))]


def items():
    out = []
    for i in range(NROWS):
        f, (d, a) = fam(i), row(i)
        src = f"{Z['source'][i]}-{i:03d}-{str(Z['entry'][i])[5:]}"
        out.append((src, i, f, None, ()))
        if f == "pool_fwd":
            if R.staged(d) and d["io"] == 0:
                out += [(src + "-norows", i, f, None, ("OTAL_POOL_NOROWS",)), (src + "-unaligned", i, f, "unaligned", ())]
            if d["io"]:
                out.append((src + "-fp32", i, f, "fp32", ()))
            if d["kh"] == 3 and d["sh"] == 2 and not R.staged(d):
                out.append((src + "-no133", i, f, None, ("OTAL_POOL_NO133",)))
                if d["io"] == 3:
                    out.append((src + "-argodd", i, f, "argodd", ()))
                if d["io"] == 3 and d["kt"] == 1:
                    out.append((src + "-io1", i, f, "io1", ()))
            if d["nonneg"]:
                out.append((src + "-signed", i, f, "signed", ()))
            elif d["io"] == 3 and d["kt"] == 1 and d["sh"] == 2:
                out.append((src + "-nonneg", i, f, "nonneg", ()))
        elif f == "pool_bwd":
            if R.staged(d) and d["io"] == 0:
                out += [(src + "-norows", i, f, None, ("OTAL_POOL_NOROWS",)), (src + "-unaligned", i, f, "unaligned", ())]
            if d["io"]:
                out.append((src + "-fp32", i, f, "fp32", ()))
            if d["kh"] == 3 and d["sh"] == 2 and not R.staged(d):
                out.append((src + "-no133", i, f, None, ("OTAL_POOL_NO133",)))
                if d["io"] == 3:
                    out.append((src + "-argodd", i, f, "argodd", ()))
                if d["io"] == 3 and d["kt"] == 1:
                    out.append((src + "-io1", i, f, "io1", ()))
        elif f == "gn_bwd" and (d["n_terms"] or d["dy_bs"] not in (0, d["C"] * d["T"])):
            out.append((src + "-contiguous", i, f, "contiguous", ()))
    for name, f, ints, addr in pool_extra():
        out.append(("extra-" + name, ("extra", ints, addr), f, None, ()))
    for name, f, ints in gn_extra():
        out.append((f"extra-{name}-{f}", ("extra", ints, [0] * 5), f, None, ()))
    return out


ITEMS = items()


# ------------------------------------------------------------------------------------------------ library state
@contextlib.contextmanager
def default_library():
    """The loaded library with every option at its table default (restored afterwards)."""
    from opental_amd import _lib as L
    lib = L.lib()
    saved = [(n, lib.otal_get_option(n.encode(), d)) for n, d in OPTIONS]
    for n, d in OPTIONS:
        L.set_option(n, d)
    try:
        yield lib
    finally:
        for n, v in saved:
            L.set_option(n, v)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    """pool_choose() on the CPU (tests/cpu_pool_select.cpp): the kernel each pool launch must report."""
    return PS.build(tmp_path_factory.mktemp("cpupoolselect"))


@pytest.fixture(scope="module")
def lib():
    with default_library() as lib:
        yield lib
    if WORST:
        print("\nlargest err / bound per kernel:")
        for k in sorted(WORST):
            print(f"  {k:42s} {WORST[k][0]:.4f}   ({WORST[k][1]})")
        print(f"GroupNorm forward elements within the bound of the ReLU edge: {EDGE['n']}")


def set_switches(names, on):
    from opental_amd import _lib as L
    for n in names:
        L.set_option(n, 1 if on else dict(OPTIONS)[n])


DEV = torch.device("cuda", 0)
INT = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.uint8: torch.uint8, torch.int64: torch.int64}
SENT = {torch.float32: SENT32, torch.bfloat16: SENT16, torch.uint8: SENT8}


class Buf:
    """A fresh buffer whose view of `shape` / `strides` starts at byte residue `addr` mod 16, sentinel bits elsewhere."""

    def __init__(self, dtype, shape, strides, addr=0):
        esz = torch.empty((), dtype=dtype).element_size()
        assert addr % esz == 0, (addr, dtype)
        self.off = addr // esz
        n = sum((s - 1) * st for s, st in zip(shape, strides)) + 1
        self.base = torch.empty(self.off + n + GUARD, dtype=dtype, device=DEV)
        self.base.view(INT[dtype]).fill_(SENT[dtype])
        self.shape, self.strides, self.dtype = tuple(shape), tuple(strides), dtype
        self.view = self.base.as_strided(self.shape, self.strides, self.off)
        assert self.view.data_ptr() % 16 == addr

    def ptr(self):
        return ctypes.c_void_p(self.view.data_ptr())

    def outside_intact(self, label):
        inside = torch.zeros(self.base.numel(), dtype=torch.bool, device=DEV)
        inside.as_strided(self.shape, self.strides, self.off).fill_(True)
        bits = self.base.view(INT[self.dtype])[~inside]
        bad = int((bits != SENT[self.dtype]).sum())
        assert bad == 0, f"{label}: {bad} elements outside the output changed"


def dense(shape):
    st, acc = [], 1
    for s in reversed(shape):
        st.append(acc)
        acc *= s
    return list(reversed(st))


def note(kern, ratio, label):
    worst = float(ratio.max()) if ratio.numel() else 0.0
    if worst > WORST.get(kern, (-1.0, ""))[0]:
        WORST[kern] = (worst, label)


def check_bound(kern, label, got, val, e, K, c, f, r):
    got = got.double()
    bound = c * U * f(K) * e + r * val.abs()
    err = (got - val).abs()
    ratio = torch.where(bound > 0, err / bound, torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    ratio = torch.where(torch.isnan(got) | torch.isnan(val), torch.full_like(err, float("inf")), ratio)
    note(kern, ratio, label)
    nbad = int((ratio > 1).sum())
    if nbad:
        j = int(ratio.argmax())
        raise AssertionError(f"{label} [{kern}]: {nbad} of {ratio.numel()} elements out of bound; worst err/bound "
                             f"{float(ratio.max()):.3g} at flat {j}: got {float(got.flatten()[j])!r} ref {float(val.flatten()[j])!r} "
                             f"bound {float(bound.flatten()[j]):.3g}")


def name_of(lib):
    return lib.otal_layer_last_kernel().decode()


# ------------------------------------------------------------------------------------------------ pools
def pool_input(d, gen, nonneg, nan, half):
    """Quantised values (ties in most windows), negative first / last planes (the padding wins), exact zeros, NaNs; >= +0
    when the call promises nonneg."""
    B, C, Ti, Hi, Wi = (d[k] for k in ("B", "C", "Ti", "Hi", "Wi"))
    x = torch.randint(-3, 3, (B, C, Ti, Hi, Wi), generator=gen, device=DEV).float() * 0.5
    x[:, :, 0] = -torch.rand((B, C, Hi, Wi), generator=gen, device=DEV) - 0.25
    if Ti > 2:
        x[:, :, -1] = -torch.rand((B, C, Hi, Wi), generator=gen, device=DEV) - 0.25
    x[:, 0, :, 0] = 0.0
    if nonneg:
        x = x.abs() + 0.0
    elif nan:
        idx = torch.randint(0, x.numel(), (3,), generator=gen, device=DEV)
        x.view(-1)[idx] = float("nan")
    if half:
        x = x.to(torch.bfloat16).float()
    return x


def pool_launch(lib, entry, ga, sa, x, y, arg, bits, io):
    from opental_amd import _lib as L
    st = L.stream()
    bp = bits.ptr() if bits is not None else None
    if entry == "otal_maxpool3d_fwd":
        return lib.otal_maxpool3d_fwd(ga, sa, x.ptr(), y.ptr(), arg.ptr(), st)
    if entry == "otal_maxpool3d_fwd_signbits":
        return lib.otal_maxpool3d_fwd_signbits(ga, sa, x.ptr(), y.ptr(), arg.ptr(), bp, st)
    if entry == "otal_maxpool3d_fwd_signbits_h":
        return lib.otal_maxpool3d_fwd_signbits_h(ga, sa, x.ptr(), y.ptr(), arg.ptr(), bp, st)
    return lib.otal_maxpool3d_fwd_io(ga, sa, x.ptr(), y.ptr(), arg.ptr(), bp, io, st)


def run_pool_fwd(lib, label, d, strides, addr, entry, io, nonneg, has_bits, switches, gen, expect):
    B, C = d["B"], d["C"]
    xs, ys = [B, C, d["Ti"], d["Hi"], d["Wi"]], [B, C, d["To"], d["Ho"], d["Wo"]]
    x_st = [strides[0], strides[1]] + dense(xs[2:])
    y_st = [strides[2], strides[3]] + dense(ys[2:])
    xh, yh = bool(io & 1), bool(io & 2)
    xv = pool_input(d, gen, nonneg, nan=not nonneg, half=xh)
    x = Buf(torch.bfloat16 if xh else torch.float32, xs, x_st, addr[0])
    x.view.copy_(xv)
    y = Buf(torch.bfloat16 if yh else torch.float32, ys, y_st, addr[1])
    arg = Buf(torch.uint8, ys, dense(ys), addr[2])
    nbits = B * C * d["Ti"] * (d["Hi"] // 2) * (d["Wi"] // 4)
    bits = Buf(torch.uint8, [nbits], [1], addr[3]) if has_bits else None
    ga = (ctypes.c_int * 17)(*[d[k] for k in R.GEOM])
    sa = (ctypes.c_int64 * 4)(*strides)
    set_switches(switches, True)
    try:
        rc = pool_launch(lib, entry, ga, sa, x, y, arg, bits, io | (4 if nonneg else 0))
        name = name_of(lib)
    finally:
        set_switches(switches, False)
    torch.cuda.synchronize()
    assert (rc, name) == expect, f"{label}: the library answered {(rc, name)}, pool_choose() {expect}"
    for b_ in (y, arg) + ((bits,) if bits is not None else ()):
        b_.outside_intact(label)
    if rc == E_UNSUPPORTED:
        assert name == "", name
        for b_ in (y, arg) + ((bits,) if bits is not None else ()):
            assert int((b_.view.contiguous().view(INT[b_.dtype]) != SENT[b_.dtype]).sum()) == 0, f"{label}: refused but wrote"
        return rc, name
    assert rc == 0, f"{label}: rc {rc}"
    REACHED.add(name)
    yr, wr = R.pool_fwd(x.view.float(), d)
    got = y.view.double()
    same = (got == yr) | (torch.isnan(got) & torch.isnan(yr))
    assert bool(same.all()), f"{label} [{name}]: {int((~same).sum())} of {same.numel()} outputs differ"
    bad = int((arg.view.long() != wr).sum())
    assert bad == 0, f"{label} [{name}]: {bad} winner bytes differ"
    if bits is not None:
        bad = int((bits.view.view(d["B"], d["C"], d["Ti"], d["Hi"] // 2, d["Wi"] // 4).long() != R.signbits(x.view.float(), d)).sum())
        assert bad == 0, f"{label} [{name}]: {bad} sign-bit bytes differ"
    note(name, torch.zeros(1), label)
    return rc, name


def run_pool_bwd(lib, label, d, strides, addr, entry, io, acc, has_mask, has_scale, has_bits, switches, gen, expect):
    from opental_amd import _lib as L
    B, C = d["B"], d["C"]
    xs, ys = [B, C, d["Ti"], d["Hi"], d["Wi"]], [B, C, d["To"], d["Ho"], d["Wo"]]
    x_st = [strides[0], strides[1]] + dense(xs[2:])
    y_st = [strides[2], strides[3]] + dense(ys[2:])
    dxh, dyh, mh = bool(io & 1), bool(io & 2), bool(io & 4)
    xv = pool_input(d, gen, False, nan=False, half=False)
    _, win = R.pool_fwd(xv, d)
    dyv = torch.randn(ys, generator=gen, device=DEV)
    if dyh:
        dyv = dyv.to(torch.bfloat16).float()
    dy = Buf(torch.bfloat16 if dyh else torch.float32, ys, y_st, addr[0])
    dy.view.copy_(dyv)
    arg = Buf(torch.uint8, ys, dense(ys), addr[2])
    arg.view.copy_(win.to(torch.uint8))
    dx = Buf(torch.bfloat16 if dxh else torch.float32, xs, x_st, addr[1])
    old = None
    if acc:
        old = torch.randn(xs, generator=gen, device=DEV)
        if dxh:
            old = old.to(torch.bfloat16).float()
        dx.view.copy_(old)
    else:
        dx.view.fill_(float("nan"))
    mask = maskbuf = bits = scale = None
    if has_mask:
        mv = torch.randn(xs, generator=gen, device=DEV)
        mv[:, :, :, 0] = 0.0
        maskbuf = Buf(torch.bfloat16 if mh else torch.float32, xs, x_st, addr[4])
        maskbuf.view.copy_(mv)
        mask = maskbuf.view.float() > 0
    if has_bits:
        bits_v = R.signbits(xv, d).to(torch.uint8)
        bits = Buf(torch.uint8, [bits_v.numel()], [1], addr[3])
        bits.view.copy_(bits_v.flatten())
        mask = xv > 0
    if has_scale:
        scale = torch.rand(C, generator=gen, device=DEV) + 0.5
    ga = (ctypes.c_int * 17)(*[d[k] for k in R.GEOM])
    sa = (ctypes.c_int64 * 4)(*strides)
    st = L.stream()
    sp = L.ptr(scale) if scale is not None else None
    mp = maskbuf.ptr() if maskbuf is not None else None
    bp = bits.ptr() if bits is not None else None
    set_switches(switches, True)
    try:
        if entry == "otal_maxpool3d_bwd":
            rc = lib.otal_maxpool3d_bwd(ga, sa, dy.ptr(), arg.ptr(), dx.ptr(), acc, mp, sp, st)
        elif entry == "otal_maxpool3d_bwd_signbits":
            rc = lib.otal_maxpool3d_bwd_signbits(ga, sa, dy.ptr(), arg.ptr(), dx.ptr(), acc, bp, sp, st)
        elif entry == "otal_maxpool3d_bwd_signbits_h":
            rc = lib.otal_maxpool3d_bwd_signbits_h(ga, sa, dy.ptr(), arg.ptr(), dx.ptr(), bp, sp, st)
        else:
            rc = lib.otal_maxpool3d_bwd_io(ga, sa, dy.ptr(), arg.ptr(), dx.ptr(), acc, mp, sp, bp, io, st)
        name = name_of(lib)
    finally:
        set_switches(switches, False)
    torch.cuda.synchronize()
    assert (rc, name) == expect, f"{label}: the library answered {(rc, name)}, pool_choose() {expect}"
    dx.outside_intact(label)
    if rc == E_UNSUPPORTED:
        assert name == "", name
        before = old if acc else None
        now = dx.view.float()
        assert bool(torch.isnan(now).all()) if before is None else torch.equal(now, before), f"{label}: refused but wrote"
        return rc, name
    assert rc == 0, f"{label}: rc {rc}"
    REACHED.add(name)
    got = dx.view.double()
    nan = int(torch.isnan(got).sum())
    assert nan == 0, f"{label} [{name}]: {nan} dx elements never written"
    val, e, K = R.pool_bwd(dyv, win, d, mask=mask, scale=scale, old=old)
    check_bound(name, label, got, val, e, K, C_POOL, lambda k: k, R_BF16 if dxh else R_FP32)
    return rc, name


# ------------------------------------------------------------------------------------------------ GroupNorm
def gn_inputs(B, C, T, G, gen):
    """Groups with mean >> std (1000 + N(0, 1)), a constant group (variance 0: rstd = 1/sqrt(eps)), gamma of both signs,
    beta across the ReLU edge."""
    cpg = C // G
    x = torch.randn(B, C, T, generator=gen, device=DEV) * 2 + 0.5
    x[:, :cpg] = 1000.0 + torch.randn(B, cpg, T, generator=gen, device=DEV)
    if G > 2:
        x[-1, cpg:2 * cpg] = 3.0
    gamma = torch.randn(C, generator=gen, device=DEV)
    beta = torch.randn(C, generator=gen, device=DEV) * 0.5
    return x.contiguous(), gamma, beta


def gn_forward_lib(lib, x, gamma, beta, G, eps, nlev, lev):
    from opental_amd import _lib as L
    B, C, T = x.shape
    y = torch.empty_like(x)
    stats = torch.empty(B, G, max(nlev, 1), 2, device=DEV)
    L.check(lib.otal_gn_relu_fwd(L.ptr(x), L.ptr(gamma), L.ptr(beta), L.ptr(y), L.ptr(stats), B, C, T, G, eps, 1,
                                 nlev, lev, L.stream()), "otal_gn_relu_fwd")
    return y, stats


def run_gn_fwd(lib, label, d, eps, entry, gen):
    from opental_amd import _lib as L
    B, C, T, G, nlev = d["B"], d["C"], d["T"], d["G"], d["nlev"]
    pairs = R.levels(T, nlev, [d[f"lev{i}"] for i in range(9)])
    lev = L.int_array([d[f"lev{i}"] for i in range(nlev + 1)]) if nlev > 1 else None
    n = 2 if d["pair"] else 1
    probs = [gn_inputs(B, C, T, G, gen) for _ in range(n)]
    y_bs, y_cs = (d["y_bs"], d["y_cs"]) if d["y_bs"] else (C * T, T)
    ys = [Buf(torch.float32, [B, C, T], [y_bs, y_cs, 1], 0) for _ in range(n)]
    for y in ys:
        y.view.fill_(float("nan"))
    stats = [Buf(torch.float32, [B, G, max(nlev, 1), 2], dense([B, G, max(nlev, 1), 2]), 0) for _ in range(n)]
    P = lambda ts: (ctypes.c_void_p * 2)(*[t.data_ptr() for t in ts])
    xs, gs, bs = [p[0] for p in probs], [p[1] for p in probs], [p[2] for p in probs]
    st = L.stream()
    if entry == "otal_gn_relu_fwd":
        rc = lib.otal_gn_relu_fwd(L.ptr(xs[0]), L.ptr(gs[0]), L.ptr(bs[0]), ys[0].ptr(), stats[0].ptr(), B, C, T, G, eps, 1, nlev, lev, st)
    elif entry == "otal_gn_relu_fwd_to":
        rc = lib.otal_gn_relu_fwd_to(L.ptr(xs[0]), L.ptr(gs[0]), L.ptr(bs[0]), ys[0].ptr(), y_bs, y_cs,
                                     stats[0].ptr(), B, C, T, G, eps, 1, nlev, lev, st)
    elif entry == "otal_gn_relu_fwd_pair":
        rc = lib.otal_gn_relu_fwd_pair(P(xs), P(gs), P(bs), P([y.view for y in ys]), P([s.view for s in stats]), B, C, T, G, eps, 1,
                                       nlev, lev, st)
    else:
        rc = lib.otal_gn_relu_fwd_pair_to(P(xs), P(gs), P(bs), P([y.view for y in ys]), y_bs, y_cs,
                                          P([s.view for s in stats]), B, C, T, G, eps, 1, nlev, lev, st)
    name = name_of(lib)
    torch.cuda.synchronize()
    assert rc == 0, f"{label}: rc {rc}"
    REACHED.add(name)
    for (x, gamma, beta), y, s in zip(probs, ys, stats):
        y.outside_intact(label)
        s.outside_intact(label)
        r = R.gn_fwd(x, gamma, beta, G, eps, 1, pairs)
        got = y.view.double()
        assert int(torch.isnan(got).sum()) == 0, f"{label}: y not written"
        bound = C_GN * U * r["K"].sqrt() * r["e_y"] + R_FP32 * r["y"].abs()
        EDGE["n"] += int((r["pre"].abs() <= bound).sum())
        check_bound(name, label + ":y", got, r["y"], r["e_y"], r["K"], C_GN, torch.sqrt, R_FP32)
        sv = s.view.double()
        Kl = r["K_stats"]
        check_bound(name, label + ":mean", sv[..., 0], r["mean"], r["e_mean"], Kl, C_GN, torch.sqrt, R_FP32)
        check_bound(name, label + ":rstd", sv[..., 1], r["rstd"], r["e_rstd"], Kl, C_GN, torch.sqrt, R_FP32)
    return rc, name


def run_gn_bwd(lib, label, d, entry, variant, gen):
    from opental_amd import _lib as L
    B, C, T, G, nlev = d["B"], d["C"], d["T"], d["G"], d["nlev"]
    eps = 1e-5
    pairs = R.levels(T, nlev, [d[f"lev{i}"] for i in range(9)])
    lev = L.int_array([d[f"lev{i}"] for i in range(nlev + 1)]) if nlev > 1 else None
    n = 2 if d["pair"] else 1
    st = L.stream()
    probs = []
    for _ in range(n):
        x, gamma, beta = gn_inputs(B, C, T, G, gen)
        y, stats = gn_forward_lib(lib, x, gamma, beta, G, eps, nlev, lev)
        probs.append((x, gamma, beta, y, stats))
    nt = d["n_terms"]
    if nt:
        terms = [(d[f"bs{k}"], d[f"cs{k}"], d[f"T{k}"]) for k in range(nt)]
    else:
        bs = d["dy_bs"] or C * T
        terms = [(bs, T, T)]
    if variant == "contiguous":
        terms = [(C * tk, tk, tk) for _, _, tk in terms]
    dys, dyv = [], []
    for p in range(n):
        row_terms, total = [], torch.zeros(B, C, T, dtype=torch.float64, device=DEV)
        tabs = torch.zeros_like(total)
        for bs_, cs_, tk in terms:
            buf = Buf(torch.float32, [B, C, tk], [bs_, cs_, 1], 0)
            v = torch.randn(B, C, tk, generator=gen, device=DEV)
            buf.view.copy_(v)
            total[:, :, :tk] += v.double()
            tabs[:, :, :tk] += v.double().abs()
            row_terms.append(buf)
        dys.append(row_terms)
        dyv.append((total, tabs))
    dx = [Buf(torch.float32, [B, C, T], dense([B, C, T]), 0) for _ in range(n)]
    part = [Buf(torch.float32, [B, 3, C], dense([B, 3, C]), 0) for _ in range(n)]
    for b_ in dx + part:
        b_.view.fill_(float("nan"))
    P = lambda ts: (ctypes.c_void_p * 2)(*[t.data_ptr() for t in ts])
    if nt:
        k = len(terms)
        rc = lib.otal_gn_relu_bwd_sum(k, (ctypes.c_void_p * k)(*[b_.view.data_ptr() for b_ in dys[0]]),
                                      (ctypes.c_int64 * k)(*[t[0] for t in terms]), (ctypes.c_int64 * k)(*[t[1] for t in terms]),
                                      (ctypes.c_int * k)(*[t[2] for t in terms]), L.ptr(probs[0][0]), L.ptr(probs[0][1]),
                                      L.ptr(probs[0][2]), L.ptr(probs[0][4]), dx[0].ptr(), part[0].ptr(), B, C, T, G, 1, nlev, lev, st)
    elif n == 2:
        rc = lib.otal_gn_relu_bwd_pair(P([dys[0][0].view, dys[1][0].view]), (ctypes.c_int64 * 2)(terms[0][0], terms[0][0]),
                                       P([p[0] for p in probs]), P([p[1] for p in probs]), P([p[2] for p in probs]),
                                       P([p[4] for p in probs]), P([b_.view for b_ in dx]), P([b_.view for b_ in part]), B, C, T, G, 1,
                                       nlev, lev, st)
    else:
        rc = lib.otal_gn_relu_bwd(dys[0][0].ptr(), terms[0][0], L.ptr(probs[0][0]), L.ptr(probs[0][1]),
                                  L.ptr(probs[0][2]), L.ptr(probs[0][4]), dx[0].ptr(), part[0].ptr(), B, C, T, G, 1, nlev, lev, st)
    name = name_of(lib)
    torch.cuda.synchronize()
    assert rc == 0, f"{label}: rc {rc}"
    REACHED.add(name)
    for p in range(n):
        x, gamma, beta, y, stats = probs[p]
        dx[p].outside_intact(label)
        part[p].outside_intact(label)
        r = R.gn_bwd(dyv[p], x, gamma, G, eps, pairs, y > 0)
        got = dx[p].view.double()
        assert int(torch.isnan(got).sum()) == 0, f"{label}: dx not written"
        check_bound(name, label + ":dx", got, r["dx"], r["e_dx"], r["K"], C_GN, torch.sqrt, R_FP32)
        gp = part[p].view.double()
        assert int(torch.isnan(gp).sum()) == 0, f"{label}: partials not written"
        check_bound(name, label + ":partial", gp, r["part"], r["e_part"], r["K_part"], C_GN, torch.sqrt, R_FP32)
    return rc, name


# ------------------------------------------------------------------------------------------------ glue
def run_sum_partials(lib, label, d, gen):
    from opental_amd import _lib as L
    n = d["n"]
    items = [(d[f"C{i}"], d[f"B{i}"]) for i in range(min(n, 32))]
    parts = [torch.randn(B, 3, C, generator=gen, device=DEV) for C, B in items]
    dst = [Buf(torch.float32, [3, C], [C, 1], 0) for C, _ in items]
    for b_ in dst:
        b_.view.fill_(float("nan"))
    VP = lambda ps: (ctypes.c_void_p * len(ps))(*ps)
    rows = [VP([b_.view[r].data_ptr() for b_ in dst]) for r in range(3)]
    rc = lib.otal_sum_partials(len(items), VP([p.data_ptr() for p in parts]), rows[0], rows[1], rows[2],
                               L.int_array([c for c, _ in items]), L.int_array([b for _, b in items]), L.stream())
    name = name_of(lib)
    torch.cuda.synchronize()
    assert rc == 0 and name == "sum_partials", (rc, name)
    for (C, B), p, b_ in zip(items, parts, dst):
        b_.outside_intact(label)
        val, e, K = R.sum_partials(p, B, C)
        check_bound(name, label, b_.view.double(), val, e, torch.full_like(val, float(K)), C_GLUE, lambda k: k, R_FP32)
    return rc, name


def special_f32(n, gen):
    sp = torch.tensor([0x7F7FFFFF, 0x7F800000, 0xFF800000, 0, 0x80000000, 1, 0x007FFFFF, 0x80400000, 0x3F808000, 0x3F818000,
                       0x3F80C000, 0x3F807FFF, 0x7F7F8000, 0x7FC00000, 0xFFC00001, 0x00008000], dtype=torch.int64)
    v = torch.randn(n, generator=gen, device=DEV)
    k = min(n, 4 * len(sp))
    v.view(torch.int32)[:k] = sp.repeat(4)[:k].to(torch.int32).to(DEV)
    return v


def run_convert(lib, label, d, addr, gen):
    from opental_amd import _lib as L
    B, C, P = d["B"], d["C"], d["P"]
    to = d["to_bf16"]
    src = Buf(torch.float32 if to else torch.bfloat16, [B, C, P], [d["src_bs"], d["src_cs"], 1], addr[0])
    dst = Buf(torch.bfloat16 if to else torch.float32, [B, C, P], [d["dst_bs"], d["dst_cs"], 1], addr[1])
    v = special_f32(B * C * P, gen).view(B, C, P)
    if to:
        src.view.copy_(v)
    else:
        src.view.view(torch.int16).copy_((R.bf16_bits(v) & 0xFFFF).to(torch.int32).to(torch.int16))
    rc = lib.otal_convert_storage(src.ptr(), d["src_bs"], d["src_cs"], dst.ptr(),
                                  d["dst_bs"], d["dst_cs"], to, B, C, P, L.stream())
    name = name_of(lib)
    torch.cuda.synchronize()
    assert rc == 0, f"{label}: rc {rc}"
    REACHED.add(name)
    dst.outside_intact(label)
    if to:
        got = dst.view.contiguous().view(torch.int16).long() & 0xFFFF
        want = R.bf16_bits(v)
        nan = R.bf16_nan(want)
        bad = int((got[~nan] != want[~nan]).sum()) + int((~R.bf16_nan(got[nan])).sum())
    else:
        got = dst.view.contiguous()
        want = R.from_bf16_bits(src.view.contiguous().view(torch.int16).long())
        bad = int(((got.view(torch.int32) != want.view(torch.int32)) & ~(torch.isnan(got) & torch.isnan(want))).sum())
    assert bad == 0, f"{label} [{name}]: {bad} conversions differ"
    note(name, torch.zeros(1), label)
    return rc, name


def run_masked(lib, label, d, addr, gen):
    from opental_amd import _lib as L
    B, C, T, S = d["B"], d["C"], d["T"], d["S"]
    mk = lambda p, a: Buf(torch.float32, [B, C, T, S], [d[p + "_b"], d[p + "_c"], d[p + "_t"], 1], a)
    src, z, dst = mk("src", addr[0]), mk("z", addr[1]), mk("dst", addr[2])
    sv = torch.randn(B, C, T, S, generator=gen, device=DEV)
    zv = torch.randn(B, C, T, S, generator=gen, device=DEV)
    zv[..., 0] = 0.0
    off = zv <= 0
    junk = torch.tensor([float("inf"), float("nan"), -float("inf")], device=DEV)
    sv[off] = junk[torch.arange(int(off.sum()), device=DEV) % 3]                # a multiply by 0 would turn these into NaN
    src.view.copy_(sv)
    z.view.copy_(zv)
    scale = torch.rand(C, generator=gen, device=DEV) + 0.5 if d["has_scale"] else None
    old = None
    if d["accumulate"]:
        old = torch.randn(B, C, T, S, generator=gen, device=DEV)
        dst.view.copy_(old)
    else:
        dst.view.fill_(float("nan"))
    I64 = lambda b_: (ctypes.c_int64 * 3)(*b_.strides[:3])
    rc = lib.otal_masked_scale_copy(src.ptr(), I64(src), z.ptr(), I64(z), L.ptr(scale) if scale is not None else None, dst.ptr(),
                                    I64(dst), d["accumulate"], B, C, T, S, L.stream())
    name = name_of(lib)
    torch.cuda.synchronize()
    assert rc == 0, f"{label}: rc {rc}"
    REACHED.add(name)
    dst.outside_intact(label)
    val, e, K = R.masked_scale_copy(sv, zv, scale, old)
    got = dst.view.double()
    if old is None:
        bad = int((got != val.float().double()).sum())
        assert bad == 0, f"{label} [{name}]: {bad} elements differ"
        note(name, torch.zeros(1), label)
    else:
        check_bound(name, label, got, val, e, torch.full_like(val, float(K)), C_GLUE, lambda k: k, R_FP32)
    return rc, name


def run_merge_fwd(lib, label, d, gen):
    from opental_amd import _lib as L
    B, C, t0, T, up = d["B"], d["C"], d["t0"], d["T"], d["up"]
    p0 = torch.randn(B, C, t0, generator=gen, device=DEV)
    p1 = torch.randn(B, C, t0 // 2, generator=gen, device=DEV)
    packed = Buf(torch.float32, [B, C, t0 + t0 // 2], [C * T, T, 1], 0)
    frame = Buf(torch.float32, [B, C, t0 * up], dense([B, C, t0 * up]), 0)
    for b_ in (packed, frame):
        b_.view.fill_(float("nan"))
    rc = lib.otal_pyramid_merge_fwd(L.ptr(p0), L.ptr(p1), packed.ptr(), frame.ptr(), B, C, t0, T, up, L.stream())
    name = name_of(lib)
    torch.cuda.synchronize()
    assert rc == 0 and name == "pyramid_merge_fwd", (rc, name)
    REACHED.add(name)
    pk, fr = R.merge_fwd(p0, p1, T, up)
    packed.outside_intact(label)
    frame.outside_intact(label)
    assert torch.equal(packed.view, pk.float()), f"{label}: packed differs"
    assert torch.equal(frame.view, fr.float()), f"{label}: frame differs"
    note(name, torch.zeros(1), label)
    return rc, name


def run_merge_bwd(lib, label, d, gen):
    from opental_amd import _lib as L
    B, C, t0, T, up = d["B"], d["C"], d["t0"], d["T"], d["up"]
    da = torch.randn(B, C, T, generator=gen, device=DEV)
    db = torch.randn(B, C, T, generator=gen, device=DEV) if d["has_db"] else None
    dframe = torch.randn(B, C, t0 * up, generator=gen, device=DEV)
    dnext = torch.randn(B, C, t0 // 2, generator=gen, device=DEV) if d["has_dnext"] else None
    dp0 = Buf(torch.float32, [B, C, t0], dense([B, C, t0]), 0)
    dp1 = Buf(torch.float32, [B, C, t0 // 2], dense([B, C, t0 // 2]), 0)
    for b_ in (dp0, dp1):
        b_.view.fill_(float("nan"))
    o = lambda t: L.ptr(t) if t is not None else None
    rc = lib.otal_pyramid_merge_bwd(L.ptr(da), o(db), L.ptr(dframe), o(dnext), dp0.ptr(), dp1.ptr(), B, C, t0, T, up, L.stream())
    name = name_of(lib)
    torch.cuda.synchronize()
    assert rc == 0 and name == "pyramid_merge_bwd", (rc, name)
    REACHED.add(name)
    (v0, e0, K0), (v1, e1, K1) = R.merge_bwd(da, db, dframe, dnext, t0, up)
    for b_, v, e, K, tag in ((dp0, v0, e0, K0, "dp0"), (dp1, v1, e1, K1, "dp1")):
        b_.outside_intact(label)
        check_bound(name, f"{label}:{tag}", b_.view.double(), v, e, torch.full_like(v, float(K)), C_GLUE, lambda k: k, R_FP32)
    return rc, name


# ------------------------------------------------------------------------------------------------ the items
def pool_call(f, d, variant):
    """(entry, io, nonneg, has_bits / mask flags) of a pool item after its variant."""
    if f == "pool_fwd":
        io, nonneg, bits = d["io"], d["nonneg"], d["has_signbits"]
        entry = "otal_maxpool3d_fwd_io" if io else ("otal_maxpool3d_fwd_signbits" if bits else "otal_maxpool3d_fwd")
        if variant == "fp32":
            io, nonneg = 0, 0
            entry = "otal_maxpool3d_fwd_signbits" if bits else "otal_maxpool3d_fwd"
        elif variant == "io1":
            io, nonneg, entry, bits = 1, 0, "otal_maxpool3d_fwd_signbits_h", 1
        elif variant == "signed":
            nonneg = 0
        elif variant == "nonneg":
            nonneg = 1
        return entry, io, nonneg, bits
    io, acc, mask, scale, bits = d["io"], d["accumulate"], d["has_mask"], d["has_scale"], d["has_signbits"]
    if variant == "fp32":
        io = 0
    elif variant == "io1":
        io, acc, mask = 1, 0, 0
        return "otal_maxpool3d_bwd_signbits_h", io, acc, 0, 1, 1
    if io:
        entry = "otal_maxpool3d_bwd_io"
    elif bits:
        entry = "otal_maxpool3d_bwd_signbits"
    else:
        entry = "otal_maxpool3d_bwd"
    return entry, io, acc, mask, scale, bits


def pool_item(item):
    """(d, strides, addr, call) of a pool item as it is launched: B clipped to two samples (samples beyond the second change
    nothing but the grid's height), the variant applied; call = pool_call()'s tuple."""
    _, i, f, variant, _ = item
    if isinstance(i, tuple):
        d, addr = R.unpack(f, i[1]), list(i[2])
    else:
        d, addr = row(i)
        d["B"] = min(d["B"], 2)
    if variant == "unaligned":
        addr = [4] * 5
    if variant == "argodd":
        addr = addr[:2] + [1] + addr[3:]
    return d, [d["x_bs"], d["x_cs"], d["y_bs"], d["y_cs"]], addr, pool_call(f, d, variant)


def pool_ints(d, strides, call):
    """The integer columns of a pool call in the layout of oracle.layer_ref.FIELDS, as passed (call[0] is the entry point)."""
    return [d[k] for k in R.GEOM] + list(strides) + [int(v) for v in call[1:]]


def run_pool(lib, H, label, f, d, strides, addr, call, switches, gen):
    """Launches the call and checks it; the return code and the kernel must be those pool_choose() answers on the CPU."""
    c = PS.choose(H, f, pool_ints(d, strides, call), addr, switches)
    expect = (c["rc"], c["kernel"])
    if f == "pool_fwd":
        entry, io, nonneg, bits = call
        return run_pool_fwd(lib, label, d, strides, addr, entry, io, nonneg, bits, switches, gen, expect)
    entry, io, acc, mask, scale, bits = call
    return run_pool_bwd(lib, label, d, strides, addr, entry, io, acc, mask, scale, bits, switches, gen, expect)


def item_seed(item):
    label, i = item[0], item[1]
    return (sum(i[1]) % 100003 if isinstance(i, tuple) else 1000 + i) + len(label)


@pytest.mark.parametrize("item", ITEMS, ids=[it[0] for it in ITEMS])
def test_layer_call(lib, harness, item):
    label, i, f, variant, switches = item
    gen = torch.Generator(device=DEV).manual_seed(item_seed(item))
    if f.startswith("pool"):
        d, strides, addr, call = pool_item(item)
        rc, name = run_pool(lib, harness, label, f, d, strides, addr, call, switches, gen)
        assert rc == 0 or variant is not None or switches, f"{label}: the recorded call was refused ({rc})"
        return
    if isinstance(i, tuple):
        d, addr, eps = R.unpack(f, i[1]), list(i[2]), 1e-5
    else:
        (d, addr), eps = row(i), float(Z["eps"][i])
    if f == "gn_fwd":
        entry = str(Z["entry"][i]) if not isinstance(i, tuple) else ("otal_gn_relu_fwd_pair" if d["pair"] else "otal_gn_relu_fwd")
        run_gn_fwd(lib, label, d, eps, entry, gen)
    elif f == "gn_bwd":
        run_gn_bwd(lib, label, d, None, variant, gen)
    elif f == "sum_partials":
        run_sum_partials(lib, label, d, gen)
    elif f == "convert":
        run_convert(lib, label, d, addr, gen)
    elif f == "masked":
        run_masked(lib, label, d, addr, gen)
    elif f == "merge_fwd":
        run_merge_fwd(lib, label, d, gen)
    else:
        run_merge_bwd(lib, label, d, gen)


# ------------------------------------------------------------------------------------------------ refusals
def pool_refusals():
    """(label, family, d, strides, addr, call): the documented pool refusals."""
    out = []
    # io = 1 (bf16 x, fp32 y) on a pool that is not a strided 3x3 pool
    d = dict(zip(R.GEOM, pool_geom((4, 6, 6), (3, 3, 3), (1, 1, 1))))
    P, Po = 4 * 36, 4 * 36
    out.append(("refuse-io1", "pool_fwd", d, [2 * P, P, 2 * Po, Po], [0] * 5, ("otal_maxpool3d_fwd_io", 1, 0, 0)))
    # accumulate into a bf16 dx of a strided pool
    d = dict(zip(R.GEOM, pool_geom((2, 8, 16), (1, 3, 3), (1, 2, 2))))
    P, Po = 2 * 8 * 16, 2 * 4 * 8
    out.append(("refuse-acc-bf16", "pool_bwd", d, [2 * P, P, 2 * Po, Po], [0] * 5, ("otal_maxpool3d_bwd_io", 3, 1, 0, 1, 1)))
    return out


def test_documented_refusals_write_nothing(lib, harness):
    from opental_amd import _lib as L
    gen = torch.Generator(device=DEV).manual_seed(5)
    st = L.stream()
    for label, f, d, strides, addr, call in pool_refusals():
        rc, name = run_pool(lib, harness, label, f, d, strides, addr, call, (), gen)
        assert rc == E_UNSUPPORTED and name == ""
    # pyramid merge: odd t0 (both directions), t0 > 1024 (backward: its level-0 row lives in LDS)
    B, C = 1, 2
    for t0, fwd in ((7, True), (7, False), (1026, False)):
        T = t0 + t0 // 2
        a = torch.zeros(B, C, T, device=DEV)
        out0 = torch.full((B, C, t0 * 2 + 8), float("nan"), device=DEV)
        out1 = torch.full((B, C, t0 * 2 + 8), float("nan"), device=DEV)
        if fwd:
            rc = lib.otal_pyramid_merge_fwd(L.ptr(a), L.ptr(a), L.ptr(out0), L.ptr(out1), B, C, t0, T, 2, st)
        else:
            fr = torch.zeros(B, C, t0 * 2, device=DEV)
            rc = lib.otal_pyramid_merge_bwd(L.ptr(a), None, L.ptr(fr), None, L.ptr(out0), L.ptr(out1), B, C, t0, T, 2, st)
        torch.cuda.synchronize()
        assert rc == E_SHAPE and name_of(lib) == "", (t0, fwd, rc)
        assert bool(torch.isnan(out0).all() and torch.isnan(out1).all())
    # GroupNorm: C % G != 0; a group map beyond the LDS (32 channels x 2000 frames x 4 bytes > 160 KB)
    for C, T, G, want in ((48, 16, 32, E_SHAPE), (32, 2000, 1, E_UNSUPPORTED)):
        x = torch.randn(1, C, T, device=DEV)
        gam, bet = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
        y = torch.full_like(x, float("nan"))
        stats = torch.full((1, G, 1, 2), float("nan"), device=DEV)
        rc = lib.otal_gn_relu_fwd(L.ptr(x), L.ptr(gam), L.ptr(bet), L.ptr(y), L.ptr(stats), 1, C, T, G, 1e-5, 1, 1,
                                  None, st)
        assert rc == want and name_of(lib) == "", (C, T, G, rc)
        dx = torch.full_like(x, float("nan"))
        part = torch.full((1, 3, C), float("nan"), device=DEV)
        rc = lib.otal_gn_relu_bwd(L.ptr(x), 0, L.ptr(x), L.ptr(gam), L.ptr(bet), L.ptr(stats), L.ptr(dx), L.ptr(part),
                                  1, C, T, G, 1, 1, None, st)
        assert rc == want and name_of(lib) == "", (C, T, G, rc)
        torch.cuda.synchronize()
        assert bool(torch.isnan(y).all() and torch.isnan(stats).all() and torch.isnan(dx).all() and torch.isnan(part).all())


def test_every_kernel_was_reached(lib):
    """Runs after the items above (file order): every pool instantiation and GroupNorm path served some item."""
    missing = [k for k in POOL_KERNELS + GN_PATHS if k not in REACHED]
    assert not missing, f"never reached: {missing}"
