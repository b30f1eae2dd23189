"""Float64 reference of the library's convolution (include/opental_hip.h: otal_conv_fwd / _dgrad / _wgrad), element by element.

Written as an explicit gather, multiply and sum: the operands are read from FLAT buffers with the record's batch and channel
strides (channel slices of concat buffers), out-of-range taps read zero, `nlev > 1` keeps taps inside their level.  It
computes a rectangle of the GEMM view of the launch -- chosen rows x chosen columns:

    mode 0 (forward)       rows: output channels co     columns: output positions  n = ((b*To + t)*Ho + h)*Wo + w
    mode 1 (data gradient) rows: input channels ci      columns: input positions   n = ((b*Ti + t)*Hi + h)*Wi + w
    mode 2 (weight grad.)  rows: output channels co     columns: weight entries    c = ci*kvol + (dt*kh + dh)*kw + dw

and returns, for every element, the value, the error scale e = sqrt(sum_k (a_k b_k)^2) of its products, and K, the number
of terms (in-range taps).  The epilogues are the library's: forward act(scale[co] * conv + shift[co]) (e scaled by
|scale|), data gradient (mask > 0) * out_scale[ci] * conv, and `start +` for accumulating launches.  Works on any torch
device; the GPU tests run it on the GPU for the product's shapes, tests/test_conv_reference_cpu.py checks it against torch
on the CPU."""
import torch

F64 = torch.float64


def unpack(geom):
    """The 28-int record as a dict (B, Cin, Cout, Ti, Hi, Wi, To, Ho, Wo, kt, kh, kw, st, sh, sw, pt, ph, pw, nlev, lev)."""
    g = [int(v) for v in geom]
    names = "B Cin Cout Ti Hi Wi To Ho Wo kt kh kw st sh sw pt ph pw nlev".split()
    d = dict(zip(names, g[:19]))
    d["lev"] = g[19:19 + d["nlev"] + 1] if d["nlev"] > 1 else [0, d["Ti"]]
    return d


def _level_bounds(g, t):
    """[lo, hi) of the level that time index t (a tensor) belongs to."""
    lo = torch.zeros_like(t)
    hi = torch.full_like(t, g["Ti"])
    if g["nlev"] > 1:
        for j in range(g["nlev"]):
            sel = t >= g["lev"][j]
            lo = torch.where(sel, torch.full_like(t, g["lev"][j]), lo)
            hi = torch.where(sel, torch.full_like(t, g["lev"][j + 1]), hi)
    return lo, hi


def _taps(g, dev):
    kv = torch.arange(g["kt"] * g["kh"] * g["kw"], device=dev)
    return kv // (g["kh"] * g["kw"]), (kv // g["kw"]) % g["kh"], kv % g["kw"]


def _decompose(n, T, H, W):
    return n // (T * H * W), (n // (H * W)) % T, (n // W) % H, n % W


def _src_of_output(g, b, to, ho, wo, dt, dh, dw):
    """Input offset (without the channel term) and validity of tap (dt, dh, dw) of output position (b, to, ho, wo);
    all arguments broadcast."""
    ti = to * g["st"] + dt - g["pt"]
    hi = ho * g["sh"] + dh - g["ph"]
    wi = wo * g["sw"] + dw - g["pw"]
    lo, up = _level_bounds(g, to + 0 * ti)
    ok = (ti >= lo) & (ti < up) & (hi >= 0) & (hi < g["Hi"]) & (wi >= 0) & (wi < g["Wi"])
    off = b * g["x_bs"] + (ti * g["Hi"] + hi) * g["Wi"] + wi
    return torch.where(ok, off, torch.zeros_like(off)), ok


def _dst_of_input(g, b, ti, hi, wi, dt, dh, dw):
    """Output offset (without the channel term) and validity of the output position that tap (dt, dh, dw) carries input
    position (b, ti, hi, wi) to."""
    def axis(i, p, k, s, ext):
        num = i + p - k
        q = torch.div(num, s, rounding_mode="floor")
        return q, (num >= 0) & (num - q * s == 0) & (q < ext)
    to, okt = axis(ti, g["pt"], dt, g["st"], g["To"])
    ho, okh = axis(hi, g["ph"], dh, g["sh"], g["Ho"])
    wo, okw = axis(wi, g["pw"], dw, g["sw"], g["Wo"])
    ok = okt & okh & okw
    if g["nlev"] > 1:
        lo, up = _level_bounds(g, ti + 0 * to)
        ok = ok & (to >= lo) & (to < up)
    off = b * g["y_bs"] + (to * g["Ho"] + ho) * g["Wo"] + wo
    return torch.where(ok, off, torch.zeros_like(off)), ok


def _gather(buf, off, ok):
    v = buf[off.reshape(-1)].reshape(off.shape).to(F64)
    return torch.where(ok, v, torch.zeros((), dtype=F64, device=v.device))


def conv_ref(geom, strides, mode, rows, cols, x=None, w=None, dy=None, scale=None, shift=None, relu=False,
             mask=None, out_scale=None, start=None, chunk=1 << 24):
    """Value, error scale e and term count K of output elements rows x cols of one launch (see the module docstring).

    geom: the 28-int record; strides: (x_bs, x_cs, y_bs, y_cs) in elements.  x / dy: FLAT buffers, element 0 at the
    pointer the launch is given (x for forward and weight gradient, dy for data and weight gradient); w: the forward-layout
    weight (Cout, Cin, kt, kh, kw) or its flat form.  rows / cols: 1-D int64 index tensors.  Forward: scale / shift
    (Cout,) or None, relu.  Data gradient: mask (FLAT, dx's layout: its strides are x's) with out_scale (Cin,), or None.
    start: the output's previous values at those elements (rows x cols) for an accumulating launch, or None.
    Returns (val, e, K), float64 tensors of shape (len(rows), len(cols))."""
    g = unpack(geom)
    g["x_bs"], g["x_cs"], g["y_bs"], g["y_cs"] = (int(s) for s in strides)
    dev = rows.device
    kvol = g["kt"] * g["kh"] * g["kw"]
    dt, dh, dw = _taps(g, dev)
    rows = rows.to(dev).long()
    cols = cols.to(dev).long()
    val = torch.zeros(len(rows), len(cols), dtype=F64, device=dev)
    esq = torch.zeros_like(val)
    nk = torch.zeros(len(cols), dtype=F64, device=dev)
    if mode in (0, 1):
        wm = w.reshape(g["Cout"], g["Cin"], kvol).to(dev)
        if mode == 0:                       # A[co, ci*kvol + tap]
            C, cs, buf, T, H, W = g["Cin"], g["x_cs"], x, g["To"], g["Ho"], g["Wo"]
            A = wm[rows].reshape(len(rows), C * kvol).to(F64)
        else:                               # A[ci, co*kvol + tap]
            C, cs, buf, T, H, W = g["Cout"], g["y_cs"], dy, g["Ti"], g["Hi"], g["Wi"]
            A = wm[:, rows].permute(1, 0, 2).reshape(len(rows), C * kvol).to(F64)
        step = max(1, chunk // (C * kvol))
        for c0 in range(0, len(cols), step):
            n = cols[c0:c0 + step]
            b, t, h, ww = _decompose(n, T, H, W)
            args = (b[None], t[None], h[None], ww[None], dt[:, None], dh[:, None], dw[:, None])
            base, ok = _src_of_output(g, *args) if mode == 0 else _dst_of_input(g, *args)      # (kvol, n)
            ch = torch.arange(C, device=dev)[:, None, None] * cs
            Bm = _gather(buf, base[None] + ch, ok[None].expand(C, -1, -1)).reshape(C * kvol, len(n))
            val[:, c0:c0 + step] = A @ Bm
            esq[:, c0:c0 + step] = (A * A) @ (Bm * Bm)
            nk[c0:c0 + step] = C * ok.sum(0).to(F64)
    else:
        ci, tap = cols // kvol, cols % kvol
        P = g["To"] * g["Ho"] * g["Wo"]
        step = max(1, chunk // max(len(cols), len(rows)))
        for k0 in range(0, g["B"] * P, step):
            k = torch.arange(k0, min(k0 + step, g["B"] * P), device=dev)
            b, t, h, ww = _decompose(k, g["To"], g["Ho"], g["Wo"])
            A = _gather(dy, (b * g["y_bs"] + ((t * g["Ho"] + h) * g["Wo"] + ww))[None] + rows[:, None] * g["y_cs"],
                        torch.ones(len(rows), len(k), dtype=torch.bool, device=dev))
            base, ok = _src_of_output(g, b[None], t[None], h[None], ww[None], dt[tap][:, None], dh[tap][:, None],
                                      dw[tap][:, None])
            Bm = _gather(x, base + ci[:, None] * g["x_cs"], ok)                     # (cols, k)
            val += A @ Bm.T
            esq += (A * A) @ (Bm * Bm).T
            nk += ok.sum(1).to(F64)
    e = esq.sqrt()
    K = nk[None].expand_as(val).clone()
    if mode == 0:
        if scale is not None:
            s = scale.to(dev)[rows].to(F64)[:, None]
            val, e = val * s, e * s.abs()
        if shift is not None:
            val = val + shift.to(dev)[rows].to(F64)[:, None]
        if relu:
            val = val.clamp_min(0)
    elif mode == 1 and mask is not None:
        b, t, h, ww = _decompose(cols, g["Ti"], g["Hi"], g["Wi"])
        moff = (b * g["x_bs"] + (t * g["Hi"] + h) * g["Wi"] + ww)[None] + rows[:, None] * g["x_cs"]
        m = (mask[moff.reshape(-1)].reshape(moff.shape).to(F64) > 0).to(F64) * out_scale.to(dev)[rows].to(F64)[:, None]
        val, e = val * m, e * m.abs()
    if start is not None:
        val = val + start.to(F64)
    return val, e, K


def output_offsets(geom, strides, mode, rows, cols):
    """Flat element offsets (rows x cols) of those outputs in the buffer the launch writes (y, dx, or the contiguous dW)."""
    g = unpack(geom)
    x_bs, x_cs, y_bs, y_cs = (int(s) for s in strides)
    rows, cols = rows.long(), cols.long()
    if mode == 0:
        b, t, h, w = _decompose(cols, g["To"], g["Ho"], g["Wo"])
        return (b * y_bs + (t * g["Ho"] + h) * g["Wo"] + w)[None] + rows[:, None] * y_cs
    if mode == 1:
        b, t, h, w = _decompose(cols, g["Ti"], g["Hi"], g["Wi"])
        return (b * x_bs + (t * g["Hi"] + h) * g["Wi"] + w)[None] + rows[:, None] * x_cs
    return rows[:, None] * (g["Cin"] * g["kt"] * g["kh"] * g["kw"]) + cols[None]
