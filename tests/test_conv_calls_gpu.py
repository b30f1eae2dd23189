"""GPU: every convolution call the model makes (tests/golden/conv_calls.npz: a THUMOS14 training step at b = 8 and b = 1, an
ActivityNet step at b = 2, an inference batch), replayed through the C ABI with the recorded geometry, strides, precision
bits, flags and pointer alignment, through EVERY kernel of its chain, and compared element by element with the float64
reference (oracle/conv_ref.py).

Options are the table defaults of options.h (OTAL_CONV_DIRECT_MINTILES = 140, not conftest's 1), so the recorded chain is
the one that runs; a step further down a chain is reached by the switches that remove the steps before it, and
otal_conv_last_kernel() must name the kernel the CPU harness (tests/cpu_conv_select.cpp) expects.  Variants per row: each
chain step, the kernel a removal switch leaves, the kernel-internal switches (Conv3d_1a's untiled kernel, the chunked
1x1x1 without its streaming form), persistent prologues refreshed through otal_conv_prologue_batch, deferred split-K
reductions, the fp32 parity path once per geometry, and `small-ws` (test_small_workspace): for each head kernel that splits
K, its recorded row with the smallest output at a workspace of its tables plus 2.5 slabs and at its tables alone
(conv_launch_shape says who serves and how large those are; bytes of the workspace past the offered size must stay untouched).

Per launch: the output view starts as NaN (or random, for the two accumulating calls) and none may remain; the rest of
the output buffer (other channels, slack, a guard tail) must keep its sentinel bits; sampled elements (every 32-row x
256-position block of the output, every 32 x 128 block of dW, the M edges at multiples of 32, borders, levels, random fill)
must satisfy |got - ref| <= C * 2^-24 * sqrt(K) * e + r * |ref| with ONE constant C for all kernels."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from oracle.conv_ref import conv_ref, output_offsets, unpack

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
Z = np.load(os.path.join(HERE, "golden", "conv_calls.npz"))
SMALL_WS = ("chunked", "conv1a_wgrad", "generic", "proj", "vector", "wgrad1d", "wgrad1x1_wide", "wgrad_direct")    # head kernels that split K
WS_BYTES = 192 << 20            # ops.WORKSPACE_BYTES
NROWS = len(Z["mode"])
MODES = ("fwd", "dgrad", "wgrad")
C_BOUND = 8.0                   # one constant for every kernel
U = 2.0 ** -24
R_BF16, R_FP32 = 2.0 ** -8, 2.0 ** -22
MAX_SAMPLES = 16384             # random fill up to about this many checked elements per launch
GUARD = 4096                    # elements of guard tail behind every output
SENTINEL_F32 = 0x7F7FBEEF      # a finite fp32 / an odd bf16 pattern nobody writes by accident
SENTINEL_BF16 = 0x7F5B
E_UNSUPPORTED = -7
REMOVE = {"proj": "OTAL_CONV_NOPROJ", "conv1d_tile": "OTAL_CONV_NO1DTILE", "proj_wgrad": "OTAL_CONV_NOPROJW",
          "wgrad_direct": "OTAL_CONV_NOWDIRECT", "wgrad1x1_wide": "OTAL_CONV_NOW1X1", "wgrad1d": "OTAL_CONV_NOW1D",
          "conv1a": "OTAL_CONV_NO1A", "conv1a_wgrad": "OTAL_CONV_NO1AW", "direct": "OTAL_CONV_NODIRECT"}
OPTIONS = [(n, int(v)) for n, v in re.findall(r'\{"(OTAL_\w+)",\s*(\d+)\}',
                                                open(os.path.join(REPO, "opental_amd", "csrc", "options.h")).read())]


def chain_steps(i):
    return [s.rstrip("*") for s in str(Z["chain"][i]).split(">")]


def kname(step):
    return "vector" if step.startswith("vector") else step


def is_stream_1x1(g, mode):
    d = unpack(g)
    P = d["To"] * d["Ho"] * d["Wo"]
    return (d["kt"], d["kh"], d["kw"], d["st"], d["sh"], d["sw"], d["nlev"]) == (1,) * 7 and P == d["Ti"] * d["Hi"] * d["Wi"] \
        and P % 128 == 0 and (d["Cin"] if mode == 0 else d["Cout"]) % 8 == 0


def variants():
    """(row, variant name, switches, precision override) for every test item."""
    out, seen_geom = [], set()
    for i in range(NROWS):
        mode = int(Z["mode"][i])
        steps = chain_steps(i)
        for j, s in enumerate(steps):
            sw = tuple(REMOVE[kname(p)] for p in steps[:j])
            out.append((i, kname(s), sw, None))
            if kname(s) == "chunked" and is_stream_1x1(Z["geom"][i], mode):
                out.append((i, "chunked-nostream", sw + ("OTAL_CONV_NO1X1STREAM",), None))
            if kname(s) == "conv1a":
                out.append((i, "conv1a-notile", sw + ("OTAL_CONV_1A_NOTILE",), None))
        if len(steps) == 1 and steps[0] in ("conv1a", "conv1a_wgrad", "direct"):
            out.append((i, "no" + steps[0], (REMOVE[steps[0]],), None))
        if mode in (0, 1) and int(Z["prologue_bytes"][i]) > 0:
            out.append((i, "prologue", (), None))
        if mode == 2:
            out.append((i, "deferred", (), None))
        key = (mode, tuple(Z["geom"][i]), tuple(Z["strides"][i]))
        if key not in seen_geom:
            seen_geom.add(key)
            out.append((i, "fp32", (), 2 if mode == 1 else 0))
    return out


VARIANTS = variants()


def item_id(v):
    i, name = v[0], v[1]
    src = str(Z["source"][i])
    k = int(np.sum(Z["source"][:i] == src))
    return f"{src}-{k:03d}-{MODES[int(Z['mode'][i])]}-{name}"


# ------------------------------------------------------------------------------------------------ the CPU plan harness
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cpuselect") / "libcpuselect.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-std=c++17",
                           "-I" + os.path.join(REPO, "opental_amd", "csrc"),
                           os.path.join(HERE, "cpu_conv_select.cpp"), "-o", out])
    H = ctypes.CDLL(out)
    H.cpu_kernel_name.restype = ctypes.c_char_p
    return H


def cpu_plan(H, i, precision, switches=()):
    """Kernel names of row i's plan (precision as given) under the switches (everything else at its default)."""
    ga = (ctypes.c_int * 28)(*[int(v) for v in Z["geom"][i]])
    sa = (ctypes.c_int64 * 4)(*[int(v) for v in Z["strides"][i]])
    ad = (ctypes.c_int64 * 5)(*[int(v) for v in Z["addr16"][i]])
    res = (ctypes.c_int * 32)()
    for n in switches:
        assert H.cpu_set_option(n.encode(), 1) == 0
    try:
        H.cpu_conv_plan(ga, sa, int(Z["mode"][i]), precision, int(Z["accumulate"][i]), int(Z["has_mask"][i]), ad, res)
    finally:
        for n, dflt in OPTIONS:
            H.cpu_set_option(n.encode(), dflt)
    return [H.cpu_kernel_name(res[2 + 3 * j]).decode() for j in range(res[0])]


def cpu_serving(H, i, precision, ws_bytes):
    """(kernel name, front bytes, slab bytes, splits) of the first step of row i's plan that a workspace of ws_bytes does
    not make refuse (conv_launch_shape, options at their defaults)."""
    ga = (ctypes.c_int * 28)(*[int(v) for v in Z["geom"][i]])
    sa = (ctypes.c_int64 * 4)(*[int(v) for v in Z["strides"][i]])
    ad = (ctypes.c_int64 * 5)(*[int(v) for v in Z["addr16"][i]])
    out = (ctypes.c_int64 * 12)()
    for step in range(8):
        n = H.cpu_launch_shape(ga, sa, int(Z["mode"][i]), precision, int(Z["accumulate"][i]), int(Z["has_mask"][i]), ad, step,
                               ctypes.c_uint64(ws_bytes), out)
        assert step < n, "no step of the plan serves"
        if not out[0]:
            return H.cpu_kernel_name(int(out[10])).decode(), int(out[1]), int(out[2]), int(out[3])
        assert out[11], "a final step refuses"


# ------------------------------------------------------------------------------------------------ library state
@pytest.fixture(scope="module")
def lib(harness):
    from opental_amd import _lib as L
    lib = L.lib()
    # the harness reproduces every recorded chain (so the library, with the same defaults, runs it)
    bad = [i for i in range(NROWS) if ">".join(cpu_plan(harness, i, int(Z["precision"][i])))
           != ">".join(kname(s) for s in chain_steps(i))]
    assert not bad, [(i, str(Z["chain"][i]), cpu_plan(harness, i, int(Z["precision"][i]))) for i in bad[:5]]
    saved = [(n, lib.otal_get_option(n.encode(), d)) for n, d in OPTIONS]
    for n, d in OPTIONS:
        L.set_option(n, d)
    yield lib
    for n, v in saved:
        L.set_option(n, v)
    if WORST:
        print("\nlargest err / bound per kernel (C = %g):" % C_BOUND)
        for k in sorted(WORST):
            print(f"  {k:22s} {WORST[k][0]:.4f}   ({WORST[k][1]})")


WORST = {}


# ------------------------------------------------------------------------------------------------ operands of a row
def extent(bs, cs, B, C, P):
    return (B - 1) * bs + (C - 1) * cs + P


def sample_rows(M, gen):
    r = {0, M - 1}
    for b0 in range(0, M, 32):
        r.add(int(gen.integers(b0, min(b0 + 32, M))))
        for d in (-1, 0, 1):
            if 0 <= b0 + d < M:
                r.add(b0 + d)
    return torch.tensor(sorted(r), dtype=torch.int64)


def sample_positions(d, B, T, H, W, gen, nrows, levels):
    P = T * H * W
    N = B * P
    c = {0, N - 1, P - 1, (B - 1) * P}
    for b0 in range(0, N, 256):
        c.add(int(gen.integers(b0, min(b0 + 256, N))))
    pos = lambda b, t, h, w: ((b * T + t) * H + h) * W + w
    for b in sorted({0, B - 1}):
        for _ in range(8):                       # every padded border face, first and last sample
            t, h, w = int(gen.integers(T)), int(gen.integers(H)), int(gen.integers(W))
            for tt, hh, ww in ((0, h, w), (T - 1, h, w), (t, 0, w), (t, H - 1, w), (t, h, 0), (t, h, W - 1)):
                c.add(pos(b, tt, hh, ww))
        for lo, hi in zip(levels[:-1], levels[1:]):
            if T == d["Ti"] and hi > lo:        # level packing (Ti == To)
                c.add(pos(b, lo, 0, 0))
                c.add(pos(b, hi - 1, 0, 0))
    extra = max(0, min(N, MAX_SAMPLES // max(nrows, 1)) - len(c))
    if extra:
        c.update(int(v) for v in gen.choice(N, size=min(extra, N), replace=False))
    return torch.tensor(sorted(c), dtype=torch.int64)


def sample_wcols(d, gen, nrows):
    kvol = d["kt"] * d["kh"] * d["kw"]
    N = d["Cin"] * kvol
    c = {0, N - 1}
    c.update(range(min(kvol, N)))                # every tap of the first and the last input channel
    c.update(range(N - kvol, N))
    for b0 in range(0, N, 128):
        c.add(int(gen.integers(b0, min(b0 + 128, N))))
        for dd in (-1, 0, 1):
            if 0 <= b0 + dd < N:
                c.add(b0 + dd)
    extra = max(0, min(N, MAX_SAMPLES // max(nrows, 1)) - len(c))
    if extra:
        c.update(int(v) for v in gen.choice(N, size=min(extra, N), replace=False))
    return torch.tensor(sorted(c), dtype=torch.int64)


class Row:
    """Operands (fp32 masters in the recorded layouts), samples and reference of one recorded call."""

    def __init__(self, i):
        self.i = i
        self.geom = [int(v) for v in Z["geom"][i]]
        self.strides = [int(v) for v in Z["strides"][i]]
        self.mode = int(Z["mode"][i])
        self.prec = int(Z["precision"][i])
        self.acc = int(Z["accumulate"][i])
        self.has_mask = int(Z["has_mask"][i])
        self.addr = [int(v) for v in Z["addr16"][i]]
        d = self.d = unpack(self.geom)
        dev = torch.device("cuda", 0)
        gen = np.random.default_rng(1000 + i)
        tg = torch.Generator(device=dev).manual_seed(2000 + i)
        x_bs, x_cs, y_bs, y_cs = self.strides
        Pi, Po = d["Ti"] * d["Hi"] * d["Wi"], d["To"] * d["Ho"] * d["Wo"]
        kvol = d["kt"] * d["kh"] * d["kw"]
        self.xn = extent(x_bs, x_cs, d["B"], d["Cin"], Pi)          # x / dx / mask buffers
        self.yn = extent(y_bs, y_cs, d["B"], d["Cout"], Po)         # y / dy buffers
        self.wn = d["Cout"] * d["Cin"] * kvol
        self.x = torch.randn(self.xn, device=dev, generator=tg) if self.mode != 1 else None
        self.dy = torch.randn(self.yn, device=dev, generator=tg) if self.mode != 0 else None
        self.w = torch.randn(self.wn, device=dev, generator=tg) / math.sqrt(d["Cin"] * kvol)
        self.w0 = torch.randn(self.wn, device=dev, generator=tg) / math.sqrt(d["Cin"] * kvol)    # prologue built from these
        self.scale = torch.rand(d["Cout"], device=dev, generator=tg) + 0.5
        self.shift = torch.randn(d["Cout"], device=dev, generator=tg)
        self.mask = torch.randn(self.xn, device=dev, generator=tg) if self.has_mask else None
        self.out_scale = torch.rand(d["Cin"], device=dev, generator=tg) + 0.5 if self.has_mask else None
        M = (d["Cout"], d["Cin"], d["Cout"])[self.mode]
        self.rows = sample_rows(M, gen)
        if self.mode == 2:
            self.cols = sample_wcols(d, gen, len(self.rows))
            self.outn, self.out_shape = self.wn, None
        elif self.mode == 0:
            self.cols = sample_positions(d, d["B"], d["To"], d["Ho"], d["Wo"], gen, len(self.rows), d["lev"])
            self.outn, self.out_shape = self.yn, ((d["B"], d["Cout"], Po), (y_bs, y_cs, 1))
        else:
            self.cols = sample_positions(d, d["B"], d["Ti"], d["Hi"], d["Wi"], gen, len(self.rows), d["lev"])
            self.outn, self.out_shape = self.xn, ((d["B"], d["Cin"], Pi), (x_bs, x_cs, 1))
        if self.out_shape is None:
            self.out_shape = ((1, 1, self.wn), (self.wn, self.wn, 1))
        self.rows, self.cols = self.rows.to(dev), self.cols.to(dev)
        self.offs = output_offsets(self.geom, self.strides, self.mode, self.rows, self.cols)
        self.start = torch.randn(self.outn, device=dev, generator=tg) if self.acc else None
        self.refs = {}

    def ref(self, rounded):
        """(conv value before relu, e, K) with bf16-rounded operands (precision bit 0) or the fp32 ones."""
        if rounded not in self.refs:
            rd = (lambda t: None if t is None else t.to(torch.bfloat16).float()) if rounded else (lambda t: t)
            start = self.start[self.offs] if self.acc else None
            self.refs[rounded] = conv_ref(self.geom, self.strides, self.mode, self.rows, self.cols, x=rd(self.x),
                                          w=rd(self.w), dy=rd(self.dy), scale=self.scale, shift=self.shift,
                                          mask=self.mask, out_scale=self.out_scale, start=start)
        return self.refs[rounded]


_ROW = {}


def get_row(i):
    if i not in _ROW:
        _ROW.clear()
        torch.cuda.empty_cache()
        _ROW[i] = Row(i)
    return _ROW[i]


def placed(master, half, addr):
    """A fresh buffer holding `master` (as bf16 when `half`), the returned view starting at byte residue `addr` mod 16."""
    esz = 2 if half else 4
    assert addr % esz == 0
    off = addr // esz
    base = torch.empty(master.numel() + 16 // esz, dtype=torch.bfloat16 if half else torch.float32, device=master.device)
    view = base[off:off + master.numel()]
    view.copy_(master)
    assert view.data_ptr() % 16 == addr
    return view


# ------------------------------------------------------------------------------------------------ one launch
def launch(lib, row, prec, relu=0, prologue=None, ws_bytes=WS_BYTES):
    """Runs row's call with precision `prec` and ws_bytes of workspace; returns (rc, kernel name, output base buffer, element
    offset of the output view, half, the workspace buffer: 256 bytes longer than what the call was offered)."""
    from opental_amd import _lib as L
    d, mode = row.d, row.mode
    ax, aw, ady, aout, amask = row.addr
    half_in, half_out, half_mask = bool(prec & 8), bool(prec & 4), bool(prec & 16)
    ga = (ctypes.c_int * 28)(*row.geom)
    sa = (ctypes.c_int64 * 4)(*row.strides)
    ws = torch.empty(ws_bytes + 256, dtype=torch.uint8, device="cuda")       # fresh per launch
    ws.fill_(0xFF)                                                           # (NaN, were anything to read it unwritten)
    w = placed(row.w, False, aw)
    if prologue is not None:
        prologue = prologue(w)
    o_half = (half_out if mode == 0 else half_in) if mode != 2 else False
    esz = 2 if o_half else 4
    off = aout // esz
    obase = torch.empty(off + row.outn + GUARD, dtype=torch.bfloat16 if o_half else torch.float32, device="cuda")
    obase.view(torch.int16 if o_half else torch.int32).fill_(SENTINEL_BF16 if o_half else SENTINEL_F32)
    shape, strides = row.out_shape
    oview = obase.as_strided(shape, strides, off)
    if row.acc:
        oview.copy_(row.start.as_strided(shape, strides, 0))
    else:
        oview.fill_(float("nan"))
    out = obase[off:]
    assert out.data_ptr() % 16 == aout
    st = L.stream()
    if mode == 0:
        x = placed(row.x, half_in, ax)
        rc = lib.otal_conv_fwd(ga, sa, L.ptr(x), L.ptr(w), L.ptr(row.scale), L.ptr(row.shift), L.ptr(out), int(relu), prec,
                               prologue, L.ptr(ws), ws_bytes, st)
    elif mode == 1:
        dy = placed(row.dy, half_out, ady)
        m = placed(row.mask, half_mask, amask) if row.has_mask else None
        rc = lib.otal_conv_dgrad(ga, sa, L.ptr(dy), L.ptr(w), L.ptr(out), row.acc, L.ptr(m) if m is not None else None,
                                 L.ptr(row.out_scale) if m is not None else None, prec, prologue, L.ptr(ws),
                                 ws_bytes, st)
    else:
        x = placed(row.x, half_in, ax)
        dy = placed(row.dy, half_out, ady)
        rc = lib.otal_conv_wgrad(ga, sa, L.ptr(x), L.ptr(dy), L.ptr(out), row.acc, prec, prologue, L.ptr(ws),
                                 ws_bytes, st)
    name = lib.otal_conv_last_kernel().decode()
    torch.cuda.synchronize()
    return rc, name, obase, off, o_half, ws


def check(row, obase, off, o_half, rounded, relu, label):
    shape, strides = row.out_shape
    oview = obase.as_strided(shape, strides, off)
    nan = int(torch.isnan(oview).sum())
    assert nan == 0, f"{label}: {nan} output elements never written"
    inside = torch.zeros(obase.numel(), dtype=torch.bool, device=obase.device)
    inside.as_strided(shape, strides, off).fill_(True)
    bits = obase.view(torch.int16 if o_half else torch.int32)[~inside]
    want = SENTINEL_BF16 if o_half else SENTINEL_F32
    bad = int((bits != want).sum())
    assert bad == 0, f"{label}: {bad} elements outside the output changed"
    val, e, K = row.ref(rounded)
    if relu:
        val = val.clamp_min(0)
    got = obase[off:][row.offs].double()
    r = R_BF16 if o_half else R_FP32
    bound = C_BOUND * U * K.sqrt() * e + r * val.abs()
    err = (got - val).abs()
    ratio = torch.where(bound > 0, err / bound, torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    ratio = torch.where(torch.isnan(got), torch.full_like(err, float("inf")), ratio)
    worst = float(ratio.max())
    kern = label.split(":")[0]
    if worst > WORST.get(kern, (-1.0, ""))[0]:
        WORST[kern] = (worst, label)
    nbad = int((ratio > 1).sum())
    if nbad:
        j = int(ratio.argmax())
        rr, cc = j // ratio.shape[1], j % ratio.shape[1]
        raise AssertionError(f"{label}: {nbad} of {ratio.numel()} samples out of bound; worst err/bound {worst:.3g} at "
                             f"row {int(row.rows[rr])} col {int(row.cols[cc])}: got {float(got[rr, cc])!r} "
                             f"ref {float(val[rr, cc])!r} bound {float(bound[rr, cc]):.3g}")


def set_switches(names, on):
    from opental_amd import _lib as L
    for n in names:
        L.set_option(n, 1 if on else dict(OPTIONS)[n])


@pytest.mark.parametrize("v", VARIANTS, ids=[item_id(v) for v in VARIANTS])
def test_recorded_call(lib, harness, v):
    from opental_amd import _lib as L
    i, name, switches, prec_override = v
    row = get_row(i)
    prec = row.prec if prec_override is None else prec_override
    rounded = bool(prec & 1)
    expect = cpu_plan(harness, i, prec, switches)
    if name not in ("fp32", "prologue", "deferred") and not name.startswith("no"):
        assert expect and expect[0] == name.split("-")[0], (name, expect)
    if not expect:              # the switch leaves no kernel for this launch: the library must refuse it as well
        set_switches(switches, True)
        try:
            rc, got = launch(lib, row, prec)[:2]
        finally:
            set_switches(switches, False)
        assert rc == E_UNSUPPORTED and got == "", (rc, got)
        return
    want = expect[0]
    pro = None
    if name == "prologue":
        nbytes = lib.otal_conv_prologue_bytes((ctypes.c_int * 28)(*row.geom), (ctypes.c_int64 * 4)(*row.strides), row.mode,
                                              prec & 3)
        assert nbytes == int(Z["prologue_bytes"][i])
        keep = []

        def pro(w):            # region built from w0, the weights then change to w1 (row.w), one batch refresh
            region = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
            desc = ctypes.create_string_buffer(lib.otal_conv_prologue_desc_bytes())
            w1 = w.clone()
            w.copy_(row.w0)
            nb = lib.otal_conv_prologue((ctypes.c_int * 28)(*row.geom), (ctypes.c_int64 * 4)(*row.strides), row.mode,
                                        L.ptr(w), prec & 3, L.ptr(region), nbytes, desc, L.stream())
            assert nb > 0, nb
            w.copy_(w1)
            descs = torch.frombuffer(bytearray(desc.raw), dtype=torch.uint8).cuda()
            starts = torch.tensor([0, nb], dtype=torch.int32, device="cuda")
            L.check(lib.otal_conv_prologue_batch(1, L.ptr(descs), L.ptr(starts), nb, L.stream()), "otal_conv_prologue_batch")
            keep.extend([region, descs, starts, w1])
            return L.ptr(region)
    set_switches(switches, True)
    try:
        if name == "deferred":
            L.check(lib.otal_conv_defer_reduces(1), "otal_conv_defer_reduces")
            try:
                rc, got, obase, off, oh, ws = launch(lib, row, prec)     # (ws holds the deferred slabs until the flush)
            finally:
                L.check(lib.otal_conv_flush_reduces(L.stream()), "otal_conv_flush_reduces")
                L.check(lib.otal_conv_defer_reduces(0), "otal_conv_defer_reduces(0)")
            torch.cuda.synchronize()
            results = [(rc, got, obase, off, oh, ws, 0)]
        else:
            results = []
            for relu in ((0, 1) if row.mode == 0 else (0,)):
                results.append(launch(lib, row, prec, relu, pro) + (relu,))
    finally:
        set_switches(switches, False)
    suffix = "-" + name.split("-")[1] if "-" in name else ""
    for rc, got, obase, off, oh, _, relu in results:
        assert rc == 0, f"launch failed: {rc}"
        assert got == want, f"served by {got!r}, the plan names {want!r}"
        check(row, obase, off, oh, rounded, relu, f"{got}{suffix}:{item_id(v)}" + (":relu" if relu else ""))


@pytest.mark.parametrize("kernel", SMALL_WS)
def test_small_workspace(lib, harness, kernel):
    """small-ws: the recorded row with the smallest output among those whose head kernel is `kernel` and splits K at 192 MiB,
    at a workspace of its tables plus 2.5 slabs and at its tables alone."""
    rows = {}
    for i in range(NROWS):
        head, _, _, splits = cpu_serving(harness, i, int(Z["precision"][i]), WS_BYTES)
        if splits > 1:
            d = unpack(Z["geom"][i])
            size = (d["Cout"] * d["B"] * d["To"] * d["Ho"] * d["Wo"], d["Cin"] * d["B"] * d["Ti"] * d["Hi"] * d["Wi"],
                    d["Cout"] * d["Cin"] * d["kt"] * d["kh"] * d["kw"])[int(Z["mode"][i])]
            assert head == kname(chain_steps(i)[0])
            rows.setdefault(head, []).append((size, i))
    assert set(rows) == set(SMALL_WS), sorted(rows)
    i = min(rows[kernel])[1]
    row = get_row(i)
    head, front, slabs, splits = cpu_serving(harness, i, row.prec, WS_BYTES)
    slab1 = slabs // splits
    for ws_bytes in (front + slab1 * 5 // 2, front):
        want, _, _, want_splits = cpu_serving(harness, i, row.prec, ws_bytes)
        # 2.5 slabs clamp the split to exactly 2 (proj: all its slabs or none; wgrad1d refuses, generic takes the 2); none: 1
        assert want_splits == (2 if ws_bytes > front and head != "proj" else 1), (want, want_splits)
        rc, got, obase, off, oh, ws = launch(lib, row, row.prec, ws_bytes=ws_bytes)
        assert rc == 0 and got == want, (rc, got, want, ws_bytes)
        assert bool((ws[ws_bytes:] == 0xFF).all()), f"{got}: wrote past a workspace of {ws_bytes} bytes"
        check(row, obase, off, oh, bool(row.prec & 1), 0, f"{got}-smallws:{kernel}-row{i}:{ws_bytes}")
