"""Float64 / exact references of the small kernels behind the last pyramid convolution (csrc/headconv.hip, heads.hip,
bce.hip, bmp.hip and the Adam kernel of misc.hip), for tests/test_head_kernels_gpu.py.  numpy and CPU torch only; closed
forms, no autograd, no library op.  tests/test_head_reference_cpu.py pins every function here to torch on the CPU.

Every result that the kernels reach through rounded arithmetic comes with an element-wise condition term e, so that a
test can accept
    |got - ref| <= C * 2^-24 * (K * e + n_f * |ref|)
K = the longest serial fp32 sum behind the element, n_f = the expf / tanhf / logf / log1pf calls on its path.  For a plain
sum e is the sum of the |terms|; where an already rounded value is pushed through a function (exp of a rounded product, the
log of a rounded mean) e carries the first-order propagation of that rounding, as written at each function.

Exact results (bit for bit): the permuting copies of head_outputs_fwd, boundary_scale, BoundaryMaxPooling forward and
backward in every dtype.
"""
import numpy as np
import torch

F64 = np.float64
BCE_EPS = float(np.float32(1e-12))      # the floor of F.binary_cross_entropy's backward is a float constant, in every dtype


def _f64(a):
    return np.asarray(a, dtype=F64)


def level_table(N, lev):
    """(lo, hi) of every position's level; lev = None or (0, ..., N)."""
    lev = (0, N) if lev is None else tuple(int(v) for v in lev)
    assert lev[0] == 0 and lev[-1] == N and all(b > a for a, b in zip(lev, lev[1:]))
    lo, hi = np.zeros(N, dtype=np.int64), np.zeros(N, dtype=np.int64)
    for a, b in zip(lev, lev[1:]):
        lo[a:b], hi[a:b] = a, b
    return lo, hi


def level_index(N, lev):
    lev = (0, N) if lev is None else tuple(int(v) for v in lev)
    idx = np.zeros(N, dtype=np.int64)
    for l, (a, b) in enumerate(zip(lev, lev[1:])):
        idx[a:b] = l
    return idx


# ------------------------------------------------------------------------------------------------ head convolutions
def _taps(a, N, lev):
    """a (B, R, N) -> (a[n - 1], a[n], a[n + 1]) with a neighbour outside the position's level read as zero."""
    lo, hi = level_table(N, lev)
    n = np.arange(N)
    left, right = np.zeros_like(a), np.zeros_like(a)
    lv, rv = n > lo, n + 1 < hi
    left[:, :, lv] = a[:, :, n[lv] - 1]
    right[:, :, rv] = a[:, :, n[rv] + 1]
    return left, a, right


def head_convs(x, w, bias, in_idx, ksize, lev):
    """SAME-padded Conv1d per head, level by level.  x: the input maps (B, C, N); w[h] (cout, C, k); bias[h] (cout) or None.
    -> (y, e): lists of (B, cout, N)."""
    ys, es = [], []
    for h, j in enumerate(in_idx):
        xj, wh, k = _f64(x[j]), _f64(w[h]), int(ksize[h])
        N = xj.shape[2]
        t = _taps(xj, N, lev) if k == 3 else (None, xj, None)
        y = np.zeros((xj.shape[0], wh.shape[0], N))
        e = np.zeros_like(y)
        for tap in range(k):
            xt = t[tap] if k == 3 else t[1]
            y += np.einsum("oc,bcn->bon", wh[:, :, tap], xt)
            e += np.einsum("oc,bcn->bon", np.abs(wh[:, :, tap]), np.abs(xt))
        if bias[h] is not None:
            y += _f64(bias[h])[None, :, None]
            e += np.abs(_f64(bias[h]))[None, :, None]
        ys.append(y)
        es.append(e)
    return ys, es


def head_convs_bwd(x, w, dy, in_idx, ksize, lev):
    """-> (dx, e_dx) per input (the sum over the heads on it; zeros for an input without a head), (dw, e_dw) and (db, e_db)
    per head.  dy[h] None = no gradient arrives (zeros)."""
    n_in = len(x)
    dxs = [np.zeros(_f64(a).shape) for a in x]
    edx = [np.zeros(_f64(a).shape) for a in x]
    dws, edw, dbs, edb = [], [], [], []
    for h, j in enumerate(in_idx):
        xj, wh, k = _f64(x[j]), _f64(w[h]), int(ksize[h])
        B, C, N = xj.shape
        g = np.zeros((B, wh.shape[0], N)) if dy[h] is None else _f64(dy[h])
        # y[n'] = sum_tap w[tap] x[n' + tap - 1]  =>  dx[n] = w[0] dy[n + 1] + w[1] dy[n] + w[2] dy[n - 1], neighbours
        # inside the level of n only
        gl, gc, gr = _taps(g, N, lev) if k == 3 else (None, g, None)
        xl, xc, xr = _taps(xj, N, lev) if k == 3 else (None, xj, None)
        gs = (gr, gc, gl) if k == 3 else (gc,)
        xs = (xl, xc, xr) if k == 3 else (xc,)
        dw, ew = np.zeros(wh.shape), np.zeros(wh.shape)
        for tap in range(k):
            dxs[j] += np.einsum("oc,bon->bcn", wh[:, :, tap], gs[tap])
            edx[j] += np.einsum("oc,bon->bcn", np.abs(wh[:, :, tap]), np.abs(gs[tap]))
            dw[:, :, tap] = np.einsum("bon,bcn->oc", g, xs[tap])
            ew[:, :, tap] = np.einsum("bon,bcn->oc", np.abs(g), np.abs(xs[tap]))
        dws.append(dw)
        edw.append(ew)
        dbs.append(g.sum(axis=(0, 2)))
        edb.append(np.abs(g).sum(axis=(0, 2)))
    assert len(dxs) == n_in
    return (dxs, edx), (dws, edw), (dbs, edb)


# ------------------------------------------------------------------------------------------------ head tails
# modes: 0 permute, 1 exp(scale_l * x) * stride_l, 2 / 3 / 4 permute + Dirichlet uncertainty with exp / relu / softplus evidence
def alpha(z, mode):
    z = _f64(z)
    if mode == 2:
        return np.exp(np.clip(z, -10.0, 10.0)) + 1.0
    if mode == 3:
        return np.maximum(z, 0.0) + 1.0
    return np.where(z > 20.0, z, np.log1p(np.exp(np.minimum(z, 20.0)))) + 1.0


def dalpha(z, mode):
    """clamp passes its gradient on the CLOSED interval; relu 0 at z <= 0; softplus exactly 1 above 20."""
    z = _f64(z)
    if mode == 2:
        return np.where((z >= -10.0) & (z <= 10.0), np.exp(z), 0.0)
    if mode == 3:
        return np.where(z > 0.0, 1.0, 0.0)
    ez = np.exp(np.minimum(z, 20.0))
    return np.where(z > 20.0, 1.0, ez / (ez + 1.0))


def edge_logits(mode, shape, rs):
    """Random fp32 logits with the decision edges of the mode's evidence function planted: +-10 and their neighbours on both
    sides (2), 0 and +-tiny (3), 20 and its neighbours (4)."""
    z = (rs.randn(*shape) * 4).astype(np.float32)
    f = np.float32
    edges = {2: [f(-10), f(10), np.nextafter(f(-10), f(-11)), np.nextafter(f(-10), f(0)), np.nextafter(f(10), f(11)), np.nextafter(f(10), f(0))],
             3: [f(0), f(-0.0), f(1e-45), f(-1e-45), np.finfo(f).tiny, -np.finfo(f).tiny],
             4: [f(20), np.nextafter(f(20), f(21)), np.nextafter(f(20), f(0)), f(25), f(-30)]}.get(mode, [])
    flat = z.reshape(-1)
    for i, e in enumerate(edges):
        flat[(i * 7) % flat.size] = e
    return z


def head_outputs_fwd(raw, modes, scales, lev, strides):
    """raw[i] (B, C, N) -> out[i] (B, N, C), e_out[i]; unct[i] (B, N) / e_unct[i] for modes >= 2 (else None).
    Mode 1: exp of the fp32-rounded product x * s: the product's rounding moves the result by |x s| |out| 2^-24, so
    e_out = |x s| |out|; modes 0, 2, 3, 4 copy (e_out = 0: exact).  unct = C / S, S a sum of C positive terms: e = |unct|."""
    outs, eouts, uncts, eun = [], [], [], []
    for r, mode in zip(raw, modes):
        r = _f64(r)
        B, C, N = r.shape
        xt = r.transpose(0, 2, 1)
        if mode == 1:
            li = level_index(N, lev)
            s = _f64(scales)[li][None, :, None]
            f = (np.ones(len(li)) if strides is None else _f64(strides)[li])[None, :, None]
            o = np.exp(xt * s) * f
            outs.append(o); eouts.append(np.abs(xt * s) * np.abs(o)); uncts.append(None); eun.append(None)
            continue
        outs.append(xt.copy()); eouts.append(np.zeros(xt.shape))
        if mode == 0:
            uncts.append(None); eun.append(None)
        else:
            u = C / alpha(xt, mode).sum(-1)
            uncts.append(u); eun.append(np.abs(u))
    return outs, eouts, uncts, eun


def head_outputs_bwd(raw, out, unct, dout, dunct, modes, scales, lev):
    """out / unct are the fp32 arrays handed to the kernel.  -> draw[i] (B, C, N), e_draw[i], dscales (nlev), e_dscales.
    dscales is None when no item has mode 1."""
    nlev = 1 if lev is None else len(lev) - 1
    draws, es = [], []
    ds, eds = np.zeros(nlev), np.zeros(nlev)
    for i, mode in enumerate(modes):
        r = _f64(raw[i])
        B, C, N = r.shape
        xt = r.transpose(0, 2, 1)
        g = np.zeros(xt.shape) if dout[i] is None else _f64(dout[i])
        if mode == 1:
            li = level_index(N, lev)
            s = _f64(scales)[li][None, :, None]
            d = g * _f64(out[i]) * s
            draws.append(d.transpose(0, 2, 1)); es.append(np.abs(d).transpose(0, 2, 1))
            t = g * _f64(out[i]) * xt
            for l in range(nlev):
                ds[l] += t[:, li == l, :].sum()
                eds[l] += np.abs(t[:, li == l, :]).sum()
            continue
        e = np.abs(g)
        d = g.copy()
        if mode >= 2 and dunct[i] is not None:
            u = _f64(unct[i])[:, :, None]
            coef = -_f64(dunct[i])[:, :, None] * u * u / C
            t = coef * dalpha(xt, mode)
            d = d + t
            # u * u, * dunct, / C, * dalpha: four roundings in front of the sum, and dalpha's own (expf | - | expf, +, /)
            e = e + (4.0 + {2: 1.0, 3: 0.0, 4: 3.0}[mode]) * np.abs(t)
        draws.append(d.transpose(0, 2, 1)); es.append(e.transpose(0, 2, 1))
    return draws, es, (ds if 1 in modes else None), eds


# ------------------------------------------------------------------------------------------------ boundary losses
def boundary_bce(x, mask, row0, step):
    """x (B, C, T), mask (B, rows, Tm) -> dict: m (B, 2, T) the channel-half means of tanh x, e_m = sum |tanh| / half;
    terms (B, 2, T) = BCE(m, y) with F.binary_cross_entropy's rules (logs clamped at -100), e_terms; dx (B, C, T) =
    d mean_{b,t} BCE / d x = (m - y) / max(m (1 - m), 1e-12) / (B T) / half * (1 - tanh^2), e_dx.
    The e of terms / dx are first-order propagations of an error e_m in m (and of 1 in forming 1 - m) through the logs and
    the quotient; dx adds the cancellation of 1 - tanh^2."""
    x = _f64(x)
    B, C, T = x.shape
    half = C // 2
    th = np.tanh(x).reshape(B, 2, half, T)
    m = th.sum(2) / half
    e_m = np.abs(th).sum(2) / half
    y = _f64(mask)[:, row0:row0 + 2, :(T - 1) * step + 1:step]
    assert y.shape == (B, 2, T)
    with np.errstate(divide="ignore", invalid="ignore"):
        lm, l1m = np.maximum(np.log(m), -100.0), np.maximum(np.log(1.0 - m), -100.0)
        terms = -(y * lm + (1.0 - y) * l1m)
        dl = np.where(m > 0, y / m, 0.0) + np.where(m < 1, (1.0 - y) / (1.0 - m), 0.0)
    e_terms = (e_m + 1.0) * dl + np.abs(y * lm) + np.abs((1.0 - y) * l1m)
    den = np.maximum(m * (1.0 - m), BCE_EPS)
    gm = (m - y) / den / (B * T) / half
    dx = (gm[:, :, None, :] * (1.0 - th * th)).reshape(B, C, T)
    free = m * (1.0 - m) > BCE_EPS
    cond = (e_m + 1.0) * (1.0 / den + np.where(free, np.abs(m - y) * (np.abs(1.0 - 2.0 * m) + 1.0) / (den * den), 0.0)) / (B * T) / half
    e_dx = (cond[:, :, None, :] * (1.0 - th * th) + np.abs(gm)[:, :, None, :] * 2.0 * th * th).reshape(B, C, T) + np.abs(dx)
    return dict(m=m, e_m=e_m, terms=terms, e_terms=e_terms, dx=dx, e_dx=e_dx, y=y)


def boundary_finish(terms, weights, B):
    """terms[i] (B, 2, T_i) -> out (2): sum_i w_i * mean_{b,t} terms_i[:, h]; e."""
    out, e = np.zeros(2), np.zeros(2)
    for t, w in zip(terms, weights):
        t, w = _f64(t), float(np.float32(w))
        out += w * t.mean(axis=(0, 2))
        e += abs(w) * np.abs(t).mean(axis=(0, 2))
    return out, e


def boundary_scale(dx, weights, g_start, g_end):
    """Exact: fp32 dx * (w * g) in that order; g = g_start on the first channel half, g_end on the second (None = 0)."""
    outs = []
    for d, w in zip(dx, weights):
        d = np.asarray(d, dtype=np.float32)
        C = d.shape[1]
        g = np.empty((1, C, 1), dtype=np.float32)
        g[:, :C // 2] = np.float32(0.0 if g_start is None else g_start)
        g[:, C // 2:] = np.float32(0.0 if g_end is None else g_end)
        outs.append(d * (np.float32(w) * g))
    return outs


# ------------------------------------------------------------------------------------------------ BoundaryMaxPooling
def _windows(seg, T):
    """clamp(trunc(seg), 0, T - 1), the truncation in float64 (so that +-3e9 clamps properly)."""
    return np.clip(np.trunc(seg.detach().double().numpy()), 0, T - 1).astype(np.int64)


def _scan(x, seg, lt):
    """Value and arg-max (index into T) of every (n, c, k): strict '>' scan from l; NaN never replaces; l > r gives in[l].
    x float64 (B, C, T) (every storage type widens exactly); lt = ((t0, t1, n0, n1), ...)."""
    B, C, T = x.shape
    N = seg.shape[1]
    val = np.empty((B, C, N))
    arg = np.empty((B, C, N), dtype=np.int64)
    half = C // 2
    for t0, t1, n0, n1 in lt:
        w = _windows(seg[:, n0:n1], t1 - t0) + t0
        for n in range(B):
            for k in range(n0, n1):
                for which, cs in ((0, slice(0, half)), (2, slice(half, C))):
                    l, r = w[n, k - n0, which], w[n, k - n0, which + 1]
                    best, a = x[n, cs, l].copy(), np.full(half, l, dtype=np.int64)
                    for i in range(l + 1, r + 1):
                        v = x[n, cs, i]
                        up = v > best                 # False for a NaN v and for a NaN best
                        best, a = np.where(up, v, best), np.where(up, i, a)
                    val[n, cs, k], arg[n, cs, k] = best, a
    return val, arg


def bmp_inputs(B, C, T, N, seed, nan=True, huge=3e9, dtype=torch.float32):
    """x (B, C, T), seg (B, N, 4), grad_out (B, C, N): random windows, plus -0.5 / T - 1 + 0.999 / +-huge bounds, windows with
    l > r, and NaN features at l, inside and at r of the first windows of sample 0."""
    rs = np.random.RandomState(seed)
    x = torch.from_numpy(rs.randn(B, C, T).astype(np.float32))
    seg = np.sort(rs.uniform(-3, T + 3, (B, N, 2, 2)), -1).reshape(B, N, 4).astype(np.float32)
    seg[:, 0] = [-0.5, T - 1 + 0.999, huge, -huge]        # [0, T-1] | l = T-1 > r = 0
    if N > 1:
        seg[:, 1] = [T - 2, 1, -huge, huge]               # l > r | the whole row
    seg = torch.from_numpy(seg)
    if nan:
        w = _windows(seg, T)
        for k in range(min(N, 6)):
            l, r = int(w[0, k, 0]), int(w[0, k, 1])
            x[0, k % (C // 2), (l, (l + r) // 2, r)[k % 3]] = float("nan")
    g = torch.from_numpy(rs.randn(B, C, N).astype(np.float32))
    return x.to(dtype), seg, g.to(dtype)


def _lt(T, N, t_start, n_start):
    if t_start is None:
        return ((0, T, 0, N),)
    assert t_start[-1] == T and n_start[-1] == N
    return tuple(zip(t_start[:-1], t_start[1:], n_start[:-1], n_start[1:]))


def bmp_fwd(x, seg, t_start=None, n_start=None, into=None):
    """x (B, C, T) float32 / bfloat16 / float16 / float64 torch, seg (B, N, 4) float32 -> out (B, C, N) of x's dtype (a
    maximum is a copy: exact).  into = (wide (B, Ctot, N), c0): a copy of `wide` with channels c0 .. c0 + C replaced."""
    val, _ = _scan(x.detach().double().numpy(), seg, _lt(x.shape[2], seg.shape[1], t_start, n_start))
    out = torch.from_numpy(val).to(x.dtype)
    if into is None:
        return out
    wide, c0 = into
    wide = wide.clone()
    wide[:, c0:c0 + x.shape[1]] = out
    return wide


def bmp_bwd(gout, x, seg, t_start=None, n_start=None, compat_ref_stride=False, c0=0):
    """grad_in[n, c, arg-max] += grad_out[n, c, k] in ascending k in the staging type (fp32; fp64 for float64), stored with
    one rounding.  gout may be wider than x along the channels (its slice c0 .. c0 + C is read).  compat_ref_stride: the
    reference launcher's row stride N inside the same buffers (N <= T): rows of N elements, the tail stays zero.
    -> (grad_in of x's dtype, sum |terms|)."""
    B, C, T = x.shape
    N = seg.shape[1]
    g = gout[:, c0:c0 + C]
    if compat_ref_stride and N != T:
        assert t_start is None and N <= T
        xv = x.reshape(-1)[:B * C * N].reshape(B, C, N)
        head, e = bmp_bwd(g, xv, seg)
        full = torch.zeros(B * C * T, dtype=x.dtype)
        efull = np.zeros(B * C * T)
        full[:B * C * N], efull[:B * C * N] = head.reshape(-1), e.reshape(-1)
        return full.reshape(B, C, T), efull.reshape(B, C, T)
    _, arg = _scan(x.detach().double().numpy(), seg, _lt(T, N, t_start, n_start))
    st = np.float64 if x.dtype == torch.float64 else np.float32
    gs = g.detach().double().numpy().astype(st)         # exact: every storage type widens into its staging type
    acc, e = np.zeros((B, C, T), dtype=st), np.zeros((B, C, T))
    bi, ci = np.meshgrid(np.arange(B), np.arange(C), indexing="ij")
    for k in range(N):
        acc[bi, ci, arg[:, :, k]] += gs[:, :, k]        # one (n, c) row each: no index repeats within a k
        e[bi, ci, arg[:, :, k]] += np.abs(gs[:, :, k].astype(F64))
    return torch.from_numpy(acc).to(x.dtype), e


# ------------------------------------------------------------------------------------------------ Adam
def adam_bias_corrections(beta1, beta2, step):
    """As otal_adam_flat: pow in double on the widened fp32 betas, rounded to float."""
    b1, b2 = float(np.float32(beta1)), float(np.float32(beta2))
    return np.float32(1.0 - b1 ** step), np.float32(np.sqrt(1.0 - b2 ** step))


def adam(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, grad_scale=1.0, bias_corr=None):
    """torch.optim.Adam's single-tensor update (L2 decay folded into the gradient) in float64 from the launch's actual fp32
    scalars.  -> (p, e_p), (m, e_m), (v, e_v); e is the running error of the kernel's operation order, one unit per fp32
    rounding (so K = 1 in the bound)."""
    p, g, m, v = _f64(p), _f64(g), _f64(m), _f64(v)
    lr, b1, b2, eps, wd, gs = (float(np.float32(s)) for s in (lr, beta1, beta2, eps, weight_decay, grad_scale))
    bc1, bc2s = (float(c) for c in (adam_bias_corrections(beta1, beta2, step) if bias_corr is None else bias_corr))
    a = g * gs; ea = np.abs(a)
    b = wd * p; eb = np.abs(b)
    gi = a + b; egi = ea + eb + np.abs(gi)
    o1, o2 = 1.0 - b1, 1.0 - b2
    d = gi - m; ed = egi + np.abs(d)
    t = d * o1; et = ed * o1 + np.abs(d) * o1 + np.abs(t)
    mi = m + t; emi = et + np.abs(mi)
    v2 = v * b2; ev2 = np.abs(v2)
    c = o2 * gi; ec = o2 * np.abs(gi) + o2 * egi + np.abs(c)
    c2 = c * gi; ec2 = ec * np.abs(gi) + np.abs(c) * egi + np.abs(c2)
    vi = v2 + c2; evi = ev2 + ec2 + np.abs(vi)
    s = np.sqrt(vi)
    es = np.where(s > 0, evi / (2.0 * np.where(s > 0, s, 1.0)), 0.0) + s
    q = s / bc2s; eq = es / bc2s + q
    den = q + eps; eden = eq + den
    r = mi / den; er = emi / den + np.abs(mi) * eden / (den * den) + np.abs(r)
    a1 = lr / bc1
    upd = a1 * r; eu = abs(a1) * np.abs(r) + abs(a1) * er + np.abs(upd)
    pn = p - upd; ep = eu + np.abs(pn)
    return (pn, ep), (mi, emi), (vi, evi)
