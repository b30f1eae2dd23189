"""GPU: the small kernels behind the last pyramid convolution -- csrc/headconv.hip, heads.hip, bce.hip, bmp.hip and the Adam
and proposal-window kernels of misc.hip -- through the C ABI (ctypes), at the sizes and values where their code takes
another path, against the float64 / exact references of oracle/head_ref.py, element by element.

Per launch: every output starts as a sentinel bit pattern with a guard in front and behind; every element that must be
written is written; unrequested parts, NULL-ed outputs, the slack of wide buffers and the guards keep their bits; a refused
call returns its code and writes nothing.

Exact (bit for bit): the permuting copies, otal_boundary_scale, BoundaryMaxPooling in four dtypes (NaN compared as NaN),
proposal windows, parts 1 then 2 against parts 3, otal_adam_flat_dev against otal_adam_flat.
Bounded, per element:   |got - ref| <= C_family * 2^-24 * (K * e + n_f * |ref|)
K = the longest serial fp32 sum behind the element, n_f = its expf / tanhf / logf / log1pf calls, e = the condition term of
the float64 reference (head_ref.py says what it holds per function).  One constant per family: the next power of two at or
above twice the worst ratio measured on an MI355X with C = 1 (printed at the end of a run: `pytest -s`):

    family      worst err / (2^-24 (K e + n_f |ref|))                                        constant
    headconv    0.753   dx of the one-row input, (B, C, N) = (9, 64, 130): K = 3                  2
    tails       0.999   draw of an exp-evidence item with dout and dunct (K = 1, e per rounding)   2
    bce         0.045   terms at C = 34, T = 33 (K = 18)                                          0.125
    adam        0.999   p at n = 4 194 311 (K = 1, e per rounding)                                2
Where e counts every rounding of a short chain (K <= 3) the unit is the worst case itself, and over 10^4 .. 10^6 elements
one of them comes within a fraction of a percent of it: a ratio near 1 is what correct rounding gives there.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

from oracle import afsd_oracle as O
from oracle import head_ref as H

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
C_FAMILY = {"headconv": 2.0, "tails": 2.0, "bce": 0.125, "adam": 2.0}
E_SHAPE, E_UNSUPPORTED = -2, -7
GUARD = 64
F32, BF16, F16, F64 = torch.float32, torch.bfloat16, torch.float16, torch.float64
INT = {F32: torch.int32, BF16: torch.int16, F16: torch.int16, F64: torch.int64}
SENT = {F32: 0x7F7FBEEF, BF16: 0x7F5B, F16: 0x7BEF, F64: 0x7FEFBEEFDEADBEEF}       # finite values no kernel here produces
DTYPE_CODE = {F32: 0, BF16: 1, F16: 2, F64: 3}
WORST = {}


@pytest.fixture(scope="module")
def lib():
    from opental_amd import _lib as L
    yield L.lib()
    if WORST:
        print("\nworst err / (2^-24 (K e + n_f |ref|)) per family, before the constant:")
        for k in sorted(WORST):
            print(f"  {k:10s} {WORST[k][0]:.4f}   ({WORST[k][1]})   constant {C_FAMILY[k]}")


def stream():
    from opental_amd import _lib as L
    return L.stream()


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
    return (t if dtype is None else t.to(dtype)).contiguous().cuda()


class Out:
    """A device buffer of `shape` filled with sentinel bits, `off` elements of guard in front and GUARD behind."""

    def __init__(self, shape, dtype=F32, off=4, init=None):
        n = int(np.prod(shape))
        self.dtype, self.off, self.n = dtype, off, n
        self.base = torch.empty(off + n + GUARD, dtype=dtype, device="cuda")
        self.base.view(INT[dtype]).fill_(SENT[dtype])
        self.t = self.base[off:off + n].view(shape)
        if init is not None:
            self.t.copy_(dev(init, dtype))

    def p(self, elem_offset=0):
        return ctypes.c_void_p(self.t.data_ptr() + int(elem_offset) * self.t.element_size())

    def fresh(self):
        """bool tensor (flat, whole buffer): the element still holds the sentinel bits"""
        return self.base.view(INT[self.dtype]) == SENT[self.dtype]

    def check(self, label, written=True):
        """written: True = every element of the view, False = none, or a bool tensor of the view's shape."""
        f = self.fresh()
        assert bool(f[:self.off].all()) and bool(f[self.off + self.n:].all()), f"{label}: a guard element changed"
        inner = f[self.off:self.off + self.n]
        if written is True:
            assert not bool(inner.any()), f"{label}: {int(inner.sum())} of {self.n} elements were not written"
        elif written is False:
            assert bool(inner.all()), f"{label}: {int((~inner).sum())} elements changed that must keep their bits"
        else:
            w = written.reshape(-1).cuda()
            assert bool((inner == ~w).all()), f"{label}: written elements differ from the expected set"

    def np(self):
        return self.t.cpu().numpy() if self.dtype in (F32, F64) else self.t.cpu()


def VP(items):
    def addr(t):
        if t is None:
            return None
        return t.t.data_ptr() if isinstance(t, Out) else t.data_ptr()
    return (ctypes.c_void_p * len(items))(*[addr(t) for t in items])


def IA(values):
    return (ctypes.c_int * len(values))(*[int(v) for v in values])


def FA(values):
    return None if values is None else (ctypes.c_float * len(values))(*[float(v) for v in values])


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    return np.array_equal(a.view(np.int32 if a.dtype == np.float32 else np.int64), b.view(np.int32 if a.dtype == np.float32 else np.int64))


def check_bound(fam, label, got, ref, e, K, nf):
    got, ref, e = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64), np.asarray(e, dtype=np.float64)
    assert got.shape == ref.shape == e.shape, (label, got.shape, ref.shape, e.shape)
    unit = U * (K * e + nf * np.abs(ref))
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(unit > 0, err / unit, np.where(err > 0, np.inf, 0.0))
    ratio = np.where(np.isnan(got) | np.isnan(ref), np.inf, ratio)
    worst = float(ratio.max()) if ratio.size else 0.0
    if worst > WORST.get(fam, (-1.0, ""))[0]:
        WORST[fam] = (worst, label)
    print(f"{label}: worst ratio {worst:.4f}")
    nbad = int((ratio > C_FAMILY[fam]).sum())
    if nbad:
        j = int(ratio.argmax())
        raise AssertionError(f"{label}: {nbad} of {ratio.size} elements out of bound; worst err / unit {worst:.3g} (constant "
                             f"{C_FAMILY[fam]}) at flat {j}: got {got.flat[j]!r} ref {ref.flat[j]!r} unit {unit.flat[j]:.3g}")


# ------------------------------------------------------------------------------------------------ head convolutions
# (in_idx, cout, ksize, n_inputs): rows on one input 17 and 2 with interleaved heads | 21, 1 and an input without a head | 16
HEADS = {
    "A": ((1, 0, 1, 0), (15, 1, 2, 1), (3, 1, 1, 3), 2),
    "B": ((2, 0, 2, 2), (15, 1, 2, 4), (3, 3, 1, 3), 3),
    "C": ((0, 0), (15, 1), (3, 1), 1),
}


def lev8(N):
    return {9: (0, 1, 2, 3, 4, 5, 6, 7, 9), 130: (0, 64, 96, 112, 120, 124, 126, 127, 130), 260: (0, 128, 192, 224, 240, 248, 252, 254, 260)}[N]


HC_CASES = [
    ((9, 16, 1), "A", None), ((9, 16, 1), "B", (0, 1)),
    ((2, 144, 7), "A", (0, 1, 3, 7)), ((2, 144, 7), "C", None),
    ((3, 48, 9), "B", (0, 1, 2, 4, 8, 9)), ((3, 48, 9), "A", lev8(9)),
    ((2, 32, 130), "A", (0, 1, 2, 4, 8, 130)), ((2, 32, 130), "C", lev8(130)),
    ((1, 16, 260), "B", (0, 1, 2, 4, 8, 260)), ((1, 16, 260), "A", None),
    ((9, 64, 130), "B", lev8(130)),             # 1170 * (12 + 21) * 4 = 154 440 bytes of weight-gradient LDS
    ((9, 64, 130), "C", (0, 1, 2, 4, 8, 130)),
]


def hc_meta(heads):
    in_idx, cout, ks, n_in = heads
    return (len(in_idx), n_in, IA(in_idx), IA(cout), IA(ks))


def hc_inputs(shape, heads, seed):
    B, C, N = shape
    in_idx, cout, ks, n_in = heads
    rs = np.random.RandomState(seed)
    x = [rs.randn(B, C, N).astype(np.float32) for _ in range(n_in)]
    w = [(rs.randn(co, C, k) / math.sqrt(C)).astype(np.float32) for co, k in zip(cout, ks)]
    bias = [None if h == 1 else rs.randn(co).astype(np.float32) for h, co in enumerate(cout)]
    dy = [rs.randn(B, co, N).astype(np.float32) for co in cout]
    return x, w, bias, dy


def wgrad_K(BN):
    """p0 of head_convs_wgrad_kernel: four interleaved chains over the 16-position trips, then the tail on p0 alone"""
    return (BN // 16) * 4 + BN % 16 + 2 if BN % 4 == 0 else BN


def hc_bwd(lib, heads, shape, lev, xd, wd, dyd, parts, dx_on=None, db_on=None, outs=None):
    """One otal_head_convs_bwd_parts call into fresh (or the given) sentinel buffers; dx_on / db_on: False = pass NULL."""
    B, C, N = shape
    in_idx, cout, ks, n_in = heads
    dx, dw, db = outs or ([Out((B, C, N)) for _ in range(n_in)], [Out((co, C, k)) for co, k in zip(cout, ks)], [Out((co,)) for co in cout])
    dx_on = dx_on or [True] * n_in
    db_on = db_on or [True] * len(cout)
    nlev, la = (0, None) if lev is None else (len(lev) - 1, IA(lev))
    rc = lib.otal_head_convs_bwd_parts(*hc_meta(heads), VP(xd), VP(wd), VP(dyd), VP([d if on else None for d, on in zip(dx, dx_on)]),
                                       VP(dw), VP([d if on else None for d, on in zip(db, db_on)]), B, C, N, nlev, la, parts, stream())
    torch.cuda.synchronize()
    return rc, dx, dw, db


@pytest.mark.parametrize("shape,name,lev", HC_CASES, ids=[f"{s[0]}x{s[1]}x{s[2]}-{n}-{'none' if l is None else len(l) - 1}" for s, n, l in HC_CASES])
def test_head_convs(lib, shape, name, lev):
    B, C, N = shape
    heads = HEADS[name]
    in_idx, cout, ks, n_in = heads
    nh = len(in_idx)
    label = f"head_convs {shape} {name}"
    assert lib.otal_head_convs_supported(*hc_meta(heads), B, C, N) != 0
    x, w, bias, dy = hc_inputs(shape, heads, 100 + B + C + N)
    xd, wd, dyd = [dev(a) for a in x], [dev(a) for a in w], [dev(a) for a in dy]
    bd = [None if a is None else dev(a) for a in bias]
    nlev, la = (0, None) if lev is None else (len(lev) - 1, IA(lev))
    rows = [sum(co for j, co in zip(in_idx, cout) if j == i) for i in range(n_in)]

    # forward
    y = [Out((B, co, N)) for co in cout]
    assert lib.otal_head_convs_fwd(*hc_meta(heads), VP(xd), VP(wd), VP(bd), VP(y), B, C, N, nlev, la, stream()) == 0
    torch.cuda.synchronize()
    ys, es = H.head_convs(x, w, bias, in_idx, ks, lev)
    for h in range(nh):
        y[h].check(f"{label} y[{h}]")
        check_bound("headconv", f"{label} y[{h}]", y[h].np(), ys[h], es[h], -(-C // 16) * ks[h] + 5, 0)

    # backward, both parts in one call
    (dxs, edx), (dws, edw), (dbs, edb) = H.head_convs_bwd(x, w, dy, in_idx, ks, lev)
    rc, dx, dw, db = hc_bwd(lib, heads, shape, lev, xd, wd, dyd, 3)
    assert rc == 0
    for j in range(n_in):
        dx[j].check(f"{label} dx[{j}]")
        check_bound("headconv", f"{label} dx[{j}]", dx[j].np(), dxs[j], edx[j], 3 * max(rows[j], 1), 0)
        if rows[j] == 0:
            assert not dx[j].np().any(), f"{label}: the input without a head must get a zero gradient"
    for h in range(nh):
        dw[h].check(f"{label} dw[{h}]")
        db[h].check(f"{label} db[{h}]")
        check_bound("headconv", f"{label} dw[{h}]", dw[h].np(), dws[h], edw[h], wgrad_K(B * N), 0)
        check_bound("headconv", f"{label} db[{h}]", db[h].np(), dbs[h], edb[h], wgrad_K(B * N), 0)

    # parts 1, then 2, into one set of buffers: each leaves the other's outputs alone, together they equal parts 3 bit for bit
    rc, dx1, dw1, db1 = hc_bwd(lib, heads, shape, lev, xd, wd, dyd, 1)
    assert rc == 0
    for t in dx1:
        t.check(f"{label} parts 1 dx")
    for t in dw1 + db1:
        t.check(f"{label} parts 1 dw / db", written=False)
    dx_before = [t.np().copy() for t in dx1]
    rc, _, _, _ = hc_bwd(lib, heads, shape, lev, xd, wd, dyd, 2, outs=(dx1, dw1, db1))
    assert rc == 0
    for a, b, c in zip(dx1, dx_before, dx):
        a.check(f"{label} parts 2 dx")
        assert same_bits(a.np(), b) and same_bits(a.np(), c.np()), f"{label}: dx of parts 1 / 2 / 3 differ"
    for a, c in zip(dw1 + db1, dw + db):
        a.check(f"{label} parts 2 dw / db")
        assert same_bits(a.np(), c.np()), f"{label}: dw / db of parts 2 and parts 3 differ"
    rc, dx2, dw2, db2 = hc_bwd(lib, heads, shape, lev, xd, wd, dyd, 2)
    assert rc == 0
    for t in dx2:
        t.check(f"{label} parts 2 alone dx", written=False)

    # NULL variants: no gradient for head 0, no dx for the last input with heads, no db for the last head
    jn = in_idx[-1]
    dy0 = [None] + dy[1:]
    (dxs0, edx0), (dws0, edw0), (dbs0, edb0) = H.head_convs_bwd(x, w, dy0, in_idx, ks, lev)
    rc, dxn, dwn, dbn = hc_bwd(lib, heads, shape, lev, xd, wd, [None] + dyd[1:], 3, dx_on=[j != jn for j in range(n_in)],
                               db_on=[h != nh - 1 for h in range(nh)])
    assert rc == 0
    for j in range(n_in):
        dxn[j].check(f"{label} NULL dx[{j}]", written=j != jn)
        if j != jn:
            check_bound("headconv", f"{label} dy[0] = NULL dx[{j}]", dxn[j].np(), dxs0[j], edx0[j], 3 * max(rows[j], 1), 0)
    for h in range(nh):
        dwn[h].check(f"{label} NULL dw[{h}]")
        dbn[h].check(f"{label} NULL db[{h}]", written=h != nh - 1)
        check_bound("headconv", f"{label} dy[0] = NULL dw[{h}]", dwn[h].np(), dws0[h], edw0[h], wgrad_K(B * N), 0)
    assert not dwn[0].np().any() and not dbn[0].np().any()


def test_head_convs_refusals_write_nothing(lib):
    # 22 output channels on one input
    heads = ((0, 0), (15, 7), (3, 1), 1)
    B, C, N = 2, 16, 9
    x, w, bias, dy = hc_inputs((B, C, N), heads, 5)
    xd, wd, dyd, bd = [dev(a) for a in x], [dev(a) for a in w], [dev(a) for a in dy], [None if a is None else dev(a) for a in bias]
    assert lib.otal_head_convs_supported(*hc_meta(heads), B, C, N) == 0
    y = [Out((B, co, N)) for co in heads[1]]
    assert lib.otal_head_convs_fwd(*hc_meta(heads), VP(xd), VP(wd), VP(bd), VP(y), B, C, N, 0, None, stream()) == E_UNSUPPORTED
    rc, dx, dw, db = hc_bwd(lib, heads, (B, C, N), None, xd, wd, dyd, 3)
    assert rc == E_UNSUPPORTED
    for t in y + dx + dw + db:
        t.check("22 rows", written=False)

    # the data gradient fits, the weight gradient does not: 2016 * (12 + 17) * 4 = 233 856 bytes of LDS
    heads = HEADS["C"]
    shape = (16, 16, 126)
    B, C, N = shape
    x, w, bias, dy = hc_inputs(shape, heads, 6)
    xd, wd, dyd = [dev(a) for a in x], [dev(a) for a in w], [dev(a) for a in dy]
    assert lib.otal_head_convs_supported(*hc_meta(heads), B, C, N) == 0
    rc, dx, dw, db = hc_bwd(lib, heads, shape, None, xd, wd, dyd, 3)
    assert rc == E_UNSUPPORTED
    for t in dx + dw + db:
        t.check("B 16 N 126 parts 3 refused", written=False)
    rc, dx, dw, db = hc_bwd(lib, heads, shape, None, xd, wd, dyd, 2)
    assert rc == E_UNSUPPORTED
    for t in dx + dw + db:
        t.check("B 16 N 126 parts 2 refused", written=False)
    # parts 1 alone is a launch that fits
    rc, dx, dw, db = hc_bwd(lib, heads, shape, None, xd, wd, dyd, 1)
    assert rc == 0
    (dxs, edx), _, _ = H.head_convs_bwd(x, w, dy, heads[0], heads[2], None)
    dx[0].check("B 16 N 126 parts 1 dx")
    check_bound("headconv", "B 16 N 126 parts 1 dx", dx[0].np(), dxs[0], edx[0], 3 * 16, 0)
    for t in dw + db:
        t.check("B 16 N 126 parts 1", written=False)


# ------------------------------------------------------------------------------------------------ head tails
TAIL_MODES = (1, 2, 0, 3, 4, 0, 2, 1)
TAIL_C = (2, 15, 1, 150, 15, 2, 150, 1)
NF_ALPHA = {2: 1, 3: 0, 4: 2}          # expf | - | expf + log1pf, per term of the evidence sum


@pytest.mark.parametrize("with_strides", [False, True], ids=["nostrides", "strides"])
@pytest.mark.parametrize("B,N,lev", [(2, 300, (0, 128, 192, 224, 240, 248, 252, 253, 300)), (3, 1, (0, 1))], ids=["N300-8lev", "N1-1lev"])
def test_head_outputs(lib, B, N, lev, with_strides):
    nlev = len(lev) - 1
    n = len(TAIL_MODES)
    rs = np.random.RandomState(N + with_strides)
    raw = [H.edge_logits(m, (B, c, N), rs) if m != 1 else (rs.randn(B, c, N) * 1.5).astype(np.float32) for m, c in zip(TAIL_MODES, TAIL_C)]
    scales = rs.uniform(0.5, 1.5, nlev).astype(np.float32)
    strides = [float(2 ** (l + 2)) for l in range(nlev)] if with_strides else None
    rawd, sd = [dev(a) for a in raw], dev(scales)
    label = f"head_outputs B {B} N {N} strides {with_strides}"
    if N > 1:
        for m, r in zip(TAIL_MODES, raw):       # the planted edges are there
            if m == 2:
                assert (r == 10).any() and (r == -10).any() and (r == np.nextafter(np.float32(10), np.float32(11))).any()
            if m == 3:
                assert (r == 0).any() and (r == np.float32(1e-45)).any()
            if m == 4:
                assert (r == 20).any() and (r == np.nextafter(np.float32(20), np.float32(21))).any()

    out = [Out((B, N, c)) for c in TAIL_C]
    unct = [Out((B, N)) for _ in TAIL_C]
    assert lib.otal_head_outputs_fwd(n, IA(TAIL_C), IA(TAIL_MODES), VP(rawd), VP(out), VP([u if m >= 2 else None for u, m in zip(unct, TAIL_MODES)]),
                                     ctypes.c_void_p(sd.data_ptr()), B, N, nlev, IA(lev), FA(strides), stream()) == 0
    torch.cuda.synchronize()
    ro, reo, ru, reu = H.head_outputs_fwd(raw, TAIL_MODES, scales, lev, strides)
    for i, (m, c) in enumerate(zip(TAIL_MODES, TAIL_C)):
        out[i].check(f"{label} out[{i}]")
        unct[i].check(f"{label} unct[{i}]", written=m >= 2)
        if m == 1:
            check_bound("tails", f"{label} out[{i}] mode 1", out[i].np(), ro[i], reo[i], 1, 2)
        else:
            assert same_bits(out[i].np(), ro[i].astype(np.float32)), f"{label}: out[{i}] is not a copy"
        if m >= 2:
            check_bound("tails", f"{label} unct[{i}] mode {m} C {c}", unct[i].np(), ru[i], reu[i], c + 2, NF_ALPHA[m])

    # backward: dout / dunct present or NULL per item, every combination over the first four launches
    outd, unctd = [o.t for o in out], [u.t for u in unct]
    out32, unct32 = [o.np() for o in out], [u.np() for u in unct]
    dout = [rs.randn(B, N, c).astype(np.float32) for c in TAIL_C]
    dunct = [rs.randn(B, N).astype(np.float32) for _ in TAIL_C]
    doutd, dunctd = [dev(a) for a in dout], [dev(a) for a in dunct]
    for launch in range(5):                     # (the fifth: no dout at all, so dscales is written as exact zeros)
        has_do = [launch < 4 and ((i + launch) & 1) == 0 for i in range(n)]
        has_du = [m >= 2 and (launch == 4 or ((i + launch) & 2) == 0) for i, m in enumerate(TAIL_MODES)]
        draw = [Out((B, c, N)) for c in TAIL_C]
        dsc = Out((nlev,))
        rc = lib.otal_head_outputs_bwd(n, IA(TAIL_C), IA(TAIL_MODES), VP(rawd), VP(outd), VP([u if m >= 2 else None for u, m in zip(unctd, TAIL_MODES)]),
                                       VP([d if on else None for d, on in zip(doutd, has_do)]), VP([d if on else None for d, on in zip(dunctd, has_du)]),
                                       VP(draw), ctypes.c_void_p(sd.data_ptr()), dsc.p(), B, N, nlev, IA(lev), FA(strides), stream())
        assert rc == 0
        torch.cuda.synchronize()
        rd, red, rds, reds = H.head_outputs_bwd(raw, out32, unct32, [d if on else None for d, on in zip(dout, has_do)],
                                                [d if on else None for d, on in zip(dunct, has_du)], TAIL_MODES, scales, lev)
        for i, m in enumerate(TAIL_MODES):
            draw[i].check(f"{label} draw[{i}]")
            check_bound("tails", f"{label} launch {launch} draw[{i}] mode {m} dout {has_do[i]} dunct {has_du[i]}", draw[i].np(), rd[i], red[i],
                        2 if m == 1 else 1, 0)
        dsc.check(f"{label} dscales")
        Kd = [sum(-(-B * (lev[l + 1] - lev[l]) * c // 256) for m, c, on in zip(TAIL_MODES, TAIL_C, has_do) if m == 1 and on) + 8 + 2 for l in range(nlev)]
        check_bound("tails", f"{label} launch {launch} dscales", dsc.np(), rds, reds * np.asarray(Kd, dtype=np.float64), 1, 0)


# ------------------------------------------------------------------------------------------------ boundary losses
def bce_case(B, C, T, step, row0, seed):
    rs = np.random.RandomState(seed)
    half = C // 2
    wide = (np.abs(rs.randn(B, C + 3, T + 5)) * 0.7).astype(np.float32)
    Tm = (T - 1) * step + 3
    mask = rs.uniform(0.05, 0.95, (B, 3, Tm)).astype(np.float32)
    nsat = 0
    for b in range(B):
        for t in range(T):
            for h in range(2):
                q = (b * T + t + 2 * h) % 8      # 0, 1: all 0.0 under y = 0, 1;  2, 3: all 20.0 under y = 0, 1
                if q < 4:
                    wide[b, 2 + h * half:2 + (h + 1) * half, 3 + t] = 0.0 if q < 2 else 20.0
                    mask[b, row0 + h, t * step] = float(q & 1)
                    nsat += 1
    return wide, mask, nsat


@pytest.mark.parametrize("C", [2, 6, 30, 34, 1056])
def test_boundary_bce(lib, C):
    half = C // 2
    combos = [(T, B) for T in (1, 17, 33) for B in (1, 3)]
    for idx, (T, B) in enumerate(combos):
        step, row0 = [(1, 0), (4, 1), (4, 0), (1, 1)][(idx + C) % 4]
        wide, mask, nsat = bce_case(B, C, T, step, row0, C + T + B)
        assert nsat > 0
        wd, md = dev(wide), dev(mask)
        x = wide[:, 2:2 + C, 3:3 + T]
        terms, dx = Out((B, 2, T)), Out((B, C, T))
        label = f"boundary_bce B {B} C {C} T {T} step {step} row0 {row0}"
        xp = ctypes.c_void_p(wd.data_ptr() + 4 * (2 * (T + 5) + 3))
        rc = lib.otal_boundary_bce(xp, (C + 3) * (T + 5), T + 5, ctypes.c_void_p(md.data_ptr()),
                                   mask.shape[1] * mask.shape[2], mask.shape[2], row0, step, terms.p(), dx.p(),
                                   B, C, T, stream())
        assert rc == 0
        torch.cuda.synchronize()
        terms.check(label + " terms")
        dx.check(label + " dx")
        r = H.boundary_bce(x, mask, row0, step)
        sat0, sat1 = r["m"] == 0, r["m"] == 1
        assert int(sat0.sum()) + int(sat1.sum()) == nsat
        K = -(-half // 16) + 16
        check_bound("bce", label + " terms", terms.np(), r["terms"], r["e_terms"], K, 2)
        check_bound("bce", label + " dx", dx.np(), r["dx"], r["e_dx"], K, 1)
        # the saturated frames exactly: the -100 log clamp and the 1e-12 floor
        got = terms.np()
        y = r["y"]
        assert (got[sat0 & (y == 0)] == 0).all() and (got[sat0 & (y == 1)] == 100).all(), label
        assert (got[sat1 & (y == 1)] == 0).all() and (got[sat1 & (y == 0)] == 100).all(), label
        g = dx.np().reshape(B, 2, half, T)
        assert (g.transpose(0, 1, 3, 2)[sat1] == 0).all(), label


@pytest.mark.parametrize("B,Ts", [(1, (1, 255, 256, 2051)), (3, (85, 1, 700, 2))])
def test_boundary_finish(lib, B, Ts):
    rs = np.random.RandomState(B)
    weights = (1.0, 0.1, 0.1, 0.25)
    terms = [rs.uniform(0, 100, (B, 2, T)).astype(np.float32) for T in Ts]
    td = [dev(a) for a in terms]
    for n in range(1, 5):
        out = Out((2,))
        assert lib.otal_boundary_finish(n, VP(td[:n]), FA(weights[:n]), IA(Ts[:n]), B, out.p(), stream()) == 0
        torch.cuda.synchronize()
        out.check(f"boundary_finish n {n}")
        ref, e = H.boundary_finish(terms[:n], weights[:n], B)
        K = max(-(-B * T // 256) for T in Ts[:n]) + 8 + 2 + n
        check_bound("bce", f"boundary_finish B {B} n {n}", out.np(), ref, e, K, 0)


@pytest.mark.parametrize("gs,ge", [(3.0, None), (None, -0.7), (1.25, 0.3)])
def test_boundary_scale_is_exact(lib, gs, ge):
    B = 3
    shapes = [(2, 1), (6, 17), (34, 33), (1056, 5)]
    weights = (1.0, 0.1, 0.1, 0.25)
    rs = np.random.RandomState(4)
    dx = [(rs.randn(B, C, T) * 10.0 ** rs.randint(-20, 12, (B, C, T))).astype(np.float32) for C, T in shapes]
    dxd = [dev(a) for a in dx]
    outs = [Out((B, C, T)) for C, T in shapes]
    gsd = None if gs is None else dev(np.float32([gs]))
    ged = None if ge is None else dev(np.float32([ge]))
    rc = lib.otal_boundary_scale(4, VP(dxd), VP(outs), FA(weights), IA([s[0] for s in shapes]), IA([s[1] for s in shapes]), B,
                                 None if gsd is None else ctypes.c_void_p(gsd.data_ptr()), None if ged is None else ctypes.c_void_p(ged.data_ptr()), stream())
    assert rc == 0
    torch.cuda.synchronize()
    ref = H.boundary_scale(dx, weights, gs, ge)
    for i, o in enumerate(outs):
        o.check(f"boundary_scale out[{i}]")
        assert same_bits(o.np(), ref[i]), f"boundary_scale map {i} {shapes[i]}"


# ------------------------------------------------------------------------------------------------ BoundaryMaxPooling
def eq_nan(got, ref, label):
    """bit-equal, NaN compared as NaN"""
    assert got.dtype == ref.dtype and got.shape == ref.shape, label
    gn, rn = torch.isnan(got), torch.isnan(ref)
    assert torch.equal(gn, rn), f"{label}: NaN positions differ"
    g, r = got.clone(), ref.clone()
    g[gn] = 0
    r[rn] = 0
    assert torch.equal(g.view(INT[got.dtype]), r.view(INT[ref.dtype])), f"{label}: {int((g.view(INT[got.dtype]) != r.view(INT[ref.dtype])).sum())} elements differ"


@pytest.mark.parametrize("dtype", [F32, BF16, F16, F64], ids=["f32", "bf16", "f16", "f64"])
@pytest.mark.parametrize("B,C,T,N", [(2, 6, 33, 7), (1, 2, 5, 300), (2, 64, 48, 40)])
def test_bmp_is_exact_in_every_dtype(lib, B, C, T, N, dtype):
    x, seg, g = H.bmp_inputs(B, C, T, N, 7 + T, dtype=dtype)
    assert torch.isnan(x).any() and (seg.abs() > 2.0 ** 31).any()
    xd, sd, gd = x.cuda(), seg.cuda(), g.cuda()
    code = DTYPE_CODE[dtype]
    label = f"bmp {dtype} {(B, C, T, N)}"
    out = Out((B, C, N), dtype)
    assert lib.otal_bmp_fwd(ctypes.c_void_p(xd.data_ptr()), ctypes.c_void_p(sd.data_ptr()), out.p(), B, C, T, N, B, code, stream()) == 0
    torch.cuda.synchronize()
    out.check(label + " fwd")
    eq_nan(out.t.cpu(), H.bmp_fwd(x, seg), label + " fwd")
    gin = Out((B, C, T), dtype)
    assert lib.otal_bmp_bwd(ctypes.c_void_p(gd.data_ptr()), ctypes.c_void_p(xd.data_ptr()), ctypes.c_void_p(sd.data_ptr()), gin.p(), B, C, T, N, B, 0,
                            code, stream()) == 0
    torch.cuda.synchronize()
    gin.check(label + " bwd")
    eq_nan(gin.t.cpu(), H.bmp_bwd(g, x, seg)[0], label + " bwd")
    # the reference launcher's row stride
    gin = Out((B, C, T), dtype)
    rc = lib.otal_bmp_bwd(ctypes.c_void_p(gd.data_ptr()), ctypes.c_void_p(xd.data_ptr()), ctypes.c_void_p(sd.data_ptr()), gin.p(), B, C, T, N, B, 1,
                          code, stream())
    torch.cuda.synchronize()
    if N > T:
        assert rc == E_SHAPE
        gin.check(label + " compat refused", written=False)
    else:
        assert rc == 0
        gin.check(label + " compat bwd")
        eq_nan(gin.t.cpu(), H.bmp_bwd(g, x, seg, compat_ref_stride=True)[0], label + " compat bwd")


def bmp_levels(C, dtype, seed):
    Ts, Ns = (32, 16, 8, 4, 2, 1), (10, 7, 5, 3, 2, 1)
    parts = [H.bmp_inputs(2, C, t, n, seed + i, dtype=dtype) for i, (t, n) in enumerate(zip(Ts, Ns))]
    x, seg, g = (torch.cat([p[i] for p in parts], d) for i, d in ((0, 2), (1, 1), (2, 2)))
    return x.contiguous(), seg.contiguous(), g.contiguous(), tuple(int(v) for v in np.cumsum((0,) + Ts)), tuple(int(v) for v in np.cumsum((0,) + Ns))


@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
def test_bmp_six_levels_packed(lib, dtype):
    B, C = 2, 16
    x, seg, g, ts, ns = bmp_levels(C, dtype, 31)
    xd, sd, gd = x.cuda(), seg.cuda(), g.cuda()
    out, gin = Out((B, C, ns[-1]), dtype), Out((B, C, ts[-1]), dtype)
    code = DTYPE_CODE[dtype]
    assert lib.otal_bmp_fwd_levels(ctypes.c_void_p(xd.data_ptr()), ctypes.c_void_p(sd.data_ptr()), out.p(), B, C, 6, IA(ts), IA(ns), code, stream()) == 0
    assert lib.otal_bmp_bwd_levels(ctypes.c_void_p(gd.data_ptr()), ctypes.c_void_p(xd.data_ptr()), ctypes.c_void_p(sd.data_ptr()), gin.p(), B, C, 6,
                                   IA(ts), IA(ns), code, stream()) == 0
    torch.cuda.synchronize()
    out.check("bmp levels fwd")
    gin.check("bmp levels bwd")
    eq_nan(out.t.cpu(), H.bmp_fwd(x, seg, ts, ns), f"bmp levels fwd {dtype}")
    eq_nan(gin.t.cpu(), H.bmp_bwd(g, x, seg, ts, ns)[0], f"bmp levels bwd {dtype}")


def test_bmp_levels_inside_a_wider_buffer(lib):
    B, C, c0 = 2, 16, 4
    x, seg, g, ts, ns = bmp_levels(C, F32, 41)
    N, T = ns[-1], ts[-1]
    xd, sd = x.cuda(), seg.cuda()
    wide = Out((B, C + 10, N))
    rc = lib.otal_bmp_fwd_levels_to(ctypes.c_void_p(xd.data_ptr()), ctypes.c_void_p(sd.data_ptr()), wide.p(c0 * N), (C + 10) * N, B, C, 6,
                                    IA(ts), IA(ns), stream())
    assert rc == 0
    torch.cuda.synchronize()
    inside = torch.zeros(B, C + 10, N, dtype=torch.bool)
    inside[:, c0:c0 + C] = True
    wide.check("bmp levels_to", written=inside)
    eq_nan(wide.t[:, c0:c0 + C].cpu().contiguous(), H.bmp_fwd(x, seg, ts, ns), "bmp levels_to")
    gw = torch.from_numpy(np.random.RandomState(3).randn(B, C + 10, N).astype(np.float32))
    gwd = gw.cuda()
    gin = Out((B, C, T))
    rc = lib.otal_bmp_bwd_levels_from(ctypes.c_void_p(gwd.data_ptr() + 4 * c0 * N), (C + 10) * N, ctypes.c_void_p(xd.data_ptr()),
                                      ctypes.c_void_p(sd.data_ptr()), gin.p(), B, C, 6, IA(ts), IA(ns), stream())
    assert rc == 0
    torch.cuda.synchronize()
    gin.check("bmp levels_from")
    eq_nan(gin.t.cpu(), H.bmp_bwd(gw, x, seg, ts, ns, c0=c0)[0], "bmp levels_from")
    # a pooled stride below C * N is refused
    wide = Out((B, C + 10, N))
    assert lib.otal_bmp_fwd_levels_to(ctypes.c_void_p(xd.data_ptr()), ctypes.c_void_p(sd.data_ptr()), wide.p(), C * N - 1, B, C, 6,
                                      IA(ts), IA(ns), stream()) == E_SHAPE
    torch.cuda.synchronize()
    wide.check("bmp levels_to refused", written=False)


# ------------------------------------------------------------------------------------------------ Adam
ADAM_CASES = [(n, (4, 4, 4, 4), wd, step) for n in (1, 3, 1029) for wd in (0.0, 1e-3) for step in (1, 2, 100000)] + \
             [(4 * 1048576 + 7, (4, 4, 4, 4), 1e-3, 2)] + \
             [(1048576 + 5, tuple(5 if i == k else 4 for i in range(4)), 1e-3 if k & 1 else 0.0, (1, 2, 100000, 2)[k]) for k in range(4)]


@pytest.mark.parametrize("n,offs,wd,step", ADAM_CASES, ids=[f"n{n}-off{''.join(str(o - 4) for o in offs)}-wd{wd}-step{step}" for n, offs, wd, step in ADAM_CASES])
def test_adam(lib, n, offs, wd, step):
    rs = np.random.RandomState(n % 1000 + step % 7)
    lr, b1, b2, eps, gs = 1e-3, 0.9, 0.999, 1e-8, 0.5
    p0, g0 = rs.randn(n).astype(np.float32), rs.randn(n).astype(np.float32)
    m0 = (rs.randn(n) * 0.1).astype(np.float32) if step > 1 else np.zeros(n, dtype=np.float32)
    v0 = (rs.randn(n) ** 2 * 0.01).astype(np.float32) if step > 1 else np.zeros(n, dtype=np.float32)
    g0[::97] = 0.0
    if step > 1:
        m0[::97], v0[::97] = 0.0, 0.0           # an element with nothing to move: the denominator is eps alone
    label = f"adam n {n} offsets {offs} wd {wd} step {step}"

    def buffers():
        return [Out((n,), off=o, init=a) for o, a in zip(offs, (p0, g0, m0, v0))]

    p, g, m, v = buffers()
    for t, o in zip((p, g, m, v), offs):
        assert t.t.data_ptr() % 16 == (o * 4) % 16
    rc = lib.otal_adam_flat(p.p(), g.p(), m.p(), v.p(), n, lr, b1, b2,
                            eps, wd, step, gs, stream())
    assert rc == 0
    torch.cuda.synchronize()
    (rp, ep), (rm, em), (rv, ev) = H.adam(p0, g0, m0, v0, lr, b1, b2, eps, wd, step, gs)
    for t, name in ((p, "p"), (g, "g"), (m, "m"), (v, "v")):
        t.check(f"{label} {name}")              # (a sentinel left inside p, m, v is an element the sweep skipped)
    assert same_bits(g.np(), g0)
    check_bound("adam", f"{label} p", p.np(), rp, ep, 1, 0)
    check_bound("adam", f"{label} m", m.np(), rm, em, 1, 0)
    check_bound("adam", f"{label} v", v.np(), rv, ev, 1, 0)
    # the graph-replayable form, fed the same two floats
    bc = dev(np.asarray(H.adam_bias_corrections(b1, b2, step), dtype=np.float32))
    p2, g2, m2, v2 = buffers()
    rc = lib.otal_adam_flat_dev(p2.p(), g2.p(), m2.p(), v2.p(), n, lr, b1, b2,
                                eps, wd, ctypes.c_void_p(bc.data_ptr()), gs, stream())
    assert rc == 0
    torch.cuda.synchronize()
    for a, b, name in ((p, p2, "p"), (m, m2, "m"), (v, v2, "v")):
        b.check(f"{label} dev {name}")
        assert same_bits(a.np(), b.np()), f"{label}: otal_adam_flat_dev's {name} differs from otal_adam_flat's"


# ------------------------------------------------------------------------------------------------ proposal windows
def window_arguments(loc, t, frame_num):
    """The eight arguments of torch.round in O.proposal_windows and the two pairs of clamp arguments, same operation order."""
    b = loc.shape[0]
    pri = torch.Tensor([[(c + 0.5) / t] for c in range(t)]).view(-1, 1).expand(b, t, 1)
    seg = loc / frame_num * t
    centre = torch.round(pri * t - 0.5)
    plen = seg[:, :, :1] + seg[:, :, 1:]
    q4, q10 = plen / 4.0, plen / 10.0
    inner, outer = torch.clamp(q4, min=1.0), torch.clamp(q10, min=1.0)
    left, right = centre - seg[:, :, :1], centre + seg[:, :, 1:]
    return torch.cat([left - outer, left + inner, right - inner, right + outer], -1), q4, q10


def tie_counts(args):
    fl = torch.floor(args)
    tie = (args - fl) == 0.5
    even = (fl.abs() % 2) == 0
    return [(int((tie[..., i] & even[..., i]).sum()), int((tie[..., i] & ~even[..., i]).sum())) for i in range(4)]


@pytest.mark.parametrize("lens,B,frames", [((128, 64, 32, 16, 8, 4, 2, 1), 2, 256.0), ((300,), 1, 256.0), ((1,), 3, 768.0)],
                         ids=["8lev", "1lev-300", "1lev-1"])
def test_proposal_windows_on_ties_and_floors(lib, lens, B, frames):
    rs = np.random.RandomState(len(lens))
    lev = np.cumsum((0,) + lens)
    N = int(lev[-1])
    loc = np.empty((B, N, 2), dtype=np.float32)
    for i, t in enumerate(lens):
        if frames / t == int(frames / t) or t == 1:
            # level-space offsets on multiples of 1/8: l / frames * t is exact, so x.5 arguments and plen = 4, 10 do occur
            s = rs.randint(0, 97, (B, t, 2)) / 8.0
            s[:, ::3] = rs.randint(0, 8, s[:, ::3].shape) / 2.0 + 0.5              # halves: ties with the floor outer = inner = 1
            s[:, 1::5] = np.asarray([1.5, 2.5]) if t > 1 else s[:, 1::5]           # plen / 4 == 1
            s[:, 2::7] = np.asarray([4.5, 5.5]) if t > 2 else s[:, 2::7]           # plen / 10 == 1
            loc[:, lev[i]:lev[i + 1]] = (s * (frames / t)).astype(np.float32)
        else:
            loc[:, lev[i]:lev[i + 1]] = np.exp(rs.uniform(-1, 5.5, (B, t, 2))).astype(np.float32)
    if lens == (1,):
        loc[0, 0], loc[1, 0], loc[2, 0] = (0.5 * frames, 1.5 * frames), (1.5 * frames, 2.5 * frames), (4.5 * frames, 5.5 * frames)
    loc_t = torch.from_numpy(loc)
    if len(lens) > 1 or lens == (1,):
        # the constructed inputs do reach the rules, in the oracle's own arithmetic
        ties, f4, f10 = np.zeros((4, 2), dtype=np.int64), 0, 0
        for i, t in enumerate(lens):
            args, q4, q10 = window_arguments(loc_t[:, lev[i]:lev[i + 1]], t, frames)
            ties += np.asarray(tie_counts(args))
            f4 += int((q4 == 1.0).sum())
            f10 += int((q10 == 1.0).sum())
        print(f"proposal windows {lens}: ties (even, odd) per argument {ties.tolist()}, plen / 4 == 1: {f4}, plen / 10 == 1: {f10}")
        assert f4 > 0 and f10 > 0
        if len(lens) > 1:
            assert (ties > 0).all(), ties
        else:
            assert (ties.sum(1) > 0).all(), ties
    assert B * N > 256 or len(lens) == 1
    ld = dev(loc)
    seg, fseg = Out((B, N, 4)), Out((B, N, 4))
    assert lib.otal_proposal_windows(ctypes.c_void_p(ld.data_ptr()), seg.p(), fseg.p(), B, len(lens), IA(lev), frames, stream()) == 0
    torch.cuda.synchronize()
    seg.check("proposal windows seg")
    fseg.check("proposal windows frame_seg")
    for i, t in enumerate(lens):
        s_ref, f_ref = O.proposal_windows(loc_t[:, lev[i]:lev[i + 1]], t, frames)
        assert same_bits(seg.np()[:, lev[i]:lev[i + 1]], s_ref.numpy()), (lens, i)
        assert same_bits(fseg.np()[:, lev[i]:lev[i + 1]], f_ref.numpy()), (lens, i)
