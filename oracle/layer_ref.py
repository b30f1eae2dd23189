"""Float64 / exact references of the max-pool, GroupNorm + ReLU and glue kernels (csrc/pool3d.hip, gn.hip, misc.hip), for
tests/test_layer_calls_gpu.py.  Explicit gathers and sums in torch float64 / int64 on the tensors' device: no pooling,
normalisation, interpolation or dtype-conversion op of the library is used.

Which results are exact:
  * pool forward: values, winner bytes and sign bits (a maximum is a copy);
  * fp32 -> bf16 storage conversion (round to nearest even on the integer bits; a NaN stays a NaN), bf16 -> fp32;
  * the pyramid merge forward (one fp32 rounding of the exact sum of two fp32 values);
  * masked_scale_copy without accumulate (one fp32 rounding of the exact product, or exactly 0 where z <= 0).

Every summing result comes with an element-wise error scale e and a term count K; the tests accept
    |got - ref| <= C * 2^-24 * f(K) * e + r * |ref|
with one constant C per family (f and C: tests/test_layer_calls_gpu.py), r the storage rounding of the output (bf16 or fp32).

Winner bytes.  Two encodings, chosen by the geometry alone (pool_select.h is_333_s1):
  * LINEAR -- every pool except the one below: the byte holds the winner's tap (dt * kh + dh) * kw + dw, 255 when a padded
    zero won;
  * STAGED -- 3x3x3, stride 1, pad 1, To == Ti, square planes of side 12, 6 or 3 (the Inception branch pools): the maximum is
    taken separably (w, then h, then t) and the byte of position p holds three 2-bit stage taps: bits 1:0 the w tap of the
    row maximum RM[p], bits 3:2 the h tap of the plane maximum PM[p], bits 5:4 the t tap of the output at p.  The backward
    routes each gradient through the three stages.
In both the winner is the FIRST maximum in (dt, dh, dw) order with the zero padding taking part, and a NaN tap wins over
everything before it (the last NaN of the window wins, as in aten).
"""
import torch

U = 2.0 ** -24
GEOM = ("B", "C", "Ti", "Hi", "Wi", "To", "Ho", "Wo", "kt", "kh", "kw", "st", "sh", "sw", "pt", "ph", "pw")
_LEV = tuple(f"lev{i}" for i in range(9))
# the integer columns of tests/golden/layer_calls.npz per entry-point family (tools/record_layer_calls.py writes them)
FIELDS = {
    "pool_fwd": GEOM + ("x_bs", "x_cs", "y_bs", "y_cs", "io", "nonneg", "has_signbits"),
    "pool_bwd": GEOM + ("x_bs", "x_cs", "y_bs", "y_cs", "io", "accumulate", "has_mask", "has_scale", "has_signbits"),
    "gn_fwd": ("B", "C", "T", "G", "relu", "pair", "y_bs", "y_cs", "nlev") + _LEV,
    "gn_bwd": ("B", "C", "T", "G", "relu", "pair", "nlev") + _LEV + ("dy_bs", "n_terms", "bs0", "cs0", "T0", "bs1", "cs1", "T1",
                                                                      "bs2", "cs2", "T2"),
    "sum_partials": ("n",) + tuple(f"{k}{i}" for i in range(32) for k in ("C", "B")),
    "convert": ("to_bf16", "B", "C", "P", "src_bs", "src_cs", "dst_bs", "dst_cs"),
    "masked": ("B", "C", "T", "S", "accumulate", "has_scale", "src_b", "src_c", "src_t", "z_b", "z_c", "z_t", "dst_b", "dst_c",
               "dst_t"),
    "merge_fwd": ("B", "C", "t0", "T", "up"),
    "merge_bwd": ("B", "C", "t0", "T", "up", "has_db", "has_dnext"),
}
# the five address-mod-16 columns per family
ADDRS = {
    "pool_fwd": ("x", "y", "argtap", "signbits", "-"),
    "pool_bwd": ("dy", "dx", "argtap", "signbits", "mask"),
    "gn_fwd": ("x", "y", "stats", "-", "-"),
    "gn_bwd": ("dy0", "dy1", "dy2", "x", "dx"),
    "sum_partials": ("-",) * 5,
    "convert": ("src", "dst", "-", "-", "-"),
    "masked": ("src", "z", "dst", "-", "-"),
    "merge_fwd": ("p0", "p1", "packed", "frame", "-"),
    "merge_bwd": ("da", "dframe", "dp0", "dp1", "-"),
}
NINTS = max(len(v) for v in FIELDS.values())
FAMILY = {"otal_maxpool3d_fwd": "pool_fwd", "otal_maxpool3d_fwd_signbits": "pool_fwd", "otal_maxpool3d_fwd_signbits_h": "pool_fwd",
          "otal_maxpool3d_fwd_io": "pool_fwd", "otal_maxpool3d_bwd": "pool_bwd", "otal_maxpool3d_bwd_signbits": "pool_bwd",
          "otal_maxpool3d_bwd_signbits_h": "pool_bwd", "otal_maxpool3d_bwd_io": "pool_bwd", "otal_gn_relu_fwd": "gn_fwd",
          "otal_gn_relu_fwd_to": "gn_fwd", "otal_gn_relu_fwd_pair": "gn_fwd", "otal_gn_relu_fwd_pair_to": "gn_fwd",
          "otal_gn_relu_bwd": "gn_bwd", "otal_gn_relu_bwd_sum": "gn_bwd", "otal_gn_relu_bwd_pair": "gn_bwd",
          "otal_sum_partials": "sum_partials", "otal_convert_storage": "convert", "otal_masked_scale_copy": "masked",
          "otal_pyramid_merge_fwd": "merge_fwd", "otal_pyramid_merge_bwd": "merge_bwd"}


def unpack(family, ints):
    return {k: int(v) for k, v in zip(FIELDS[family], ints)}


def levels(T, nlev, lev):
    """[(lo, hi)] of a level table (nlev <= 1: one level)."""
    if nlev <= 1:
        return [(0, T)]
    return [(int(lev[i]), int(lev[i + 1])) for i in range(nlev)]


# ------------------------------------------------------------------------------------------------ max-pool
def staged(d):
    """True where the kernels write STAGED winner bytes (csrc/pool_select.h is_333_s1): the 3x3x3 / stride 1 / pad 1 pools on square
    planes of side 12, 6 or 3 with T unchanged.  Every other geometry: LINEAR bytes."""
    return (tuple(d[k] for k in ("kt", "kh", "kw", "st", "sh", "sw", "pt", "ph", "pw")) == (3, 3, 3, 1, 1, 1, 1, 1, 1)
            and d["Hi"] == d["Wi"] and d["Hi"] in (12, 6, 3) and d["To"] == d["Ti"] and d["Ho"] == d["Hi"] and d["Wo"] == d["Wi"])


def _padded(x, d):
    """x (B,C,Ti,Hi,Wi) float64 inside a zero frame that every tap of every window fits, and the mask of the inside."""
    B, C = x.shape[:2]
    size = [max(d[p] + d[i], (d[o] - 1) * d[s] + d[k]) for p, i, o, s, k in
            (("pt", "Ti", "To", "st", "kt"), ("ph", "Hi", "Ho", "sh", "kh"), ("pw", "Wi", "Wo", "sw", "kw"))]
    xp = torch.zeros((B, C, *size), dtype=torch.float64, device=x.device)
    inside = torch.zeros(size, dtype=torch.bool, device=x.device)
    sl = (slice(d["pt"], d["pt"] + d["Ti"]), slice(d["ph"], d["ph"] + d["Hi"]), slice(d["pw"], d["pw"] + d["Wi"]))
    xp[(slice(None), slice(None)) + sl] = x.double()
    inside[sl] = True
    return xp, inside


def _window(t, d, dt, dh, dw):
    """The tap (dt, dh, dw) of every window: a strided view of the padded tensor t (last three axes)."""
    return t[..., dt:dt + (d["To"] - 1) * d["st"] + 1:d["st"], dh:dh + (d["Ho"] - 1) * d["sh"] + 1:d["sh"],
             dw:dw + (d["Wo"] - 1) * d["sw"] + 1:d["sw"]]


def _first_max3(a, b, c):
    v, k = a, torch.zeros(a.shape, dtype=torch.int64, device=a.device)
    for j, w in ((1, b), (2, c)):
        take = (w > v) | torch.isnan(w)
        v, k = torch.where(take, w, v), torch.where(take, torch.full_like(k, j), k)
    return v, k


def pool_fwd(x, d):
    """(y float64 (B,C,To,Ho,Wo), winner bytes int64) of MaxPool3dSamePadding with ZERO padding; bytes in the encoding of
    staged(d)."""
    if staged(d):
        P, Ti = d["Hi"], d["Ti"]
        xp, _ = _padded(x, d)                                                   # (B, C, Ti+2, P+2, P+2)
        rm, kw_ = _first_max3(xp[..., 0:P], xp[..., 1:P + 1], xp[..., 2:P + 2])             # row maxima (.., Ti+2, P+2, P)
        pm, kh_ = _first_max3(rm[..., 0:P, :], rm[..., 1:P + 1, :], rm[..., 2:P + 2, :])    # plane maxima (.., Ti+2, P, P)
        y, kt_ = _first_max3(pm[:, :, 0:Ti], pm[:, :, 1:Ti + 1], pm[:, :, 2:Ti + 2])
        return y, kw_[:, :, 1:Ti + 1, 1:P + 1, :] | (kh_[:, :, 1:Ti + 1] << 2) | (kt_ << 4)
    xp, inside = _padded(x, d)
    best = win = None
    for dt in range(d["kt"]):
        for dh in range(d["kh"]):
            for dw in range(d["kw"]):
                v = _window(xp, d, dt, dh, dw)
                code = torch.where(_window(inside, d, dt, dh, dw), (dt * d["kh"] + dh) * d["kw"] + dw, 255).expand(v.shape)
                if best is None:
                    best, win = v.clone(), code.clone()
                else:
                    take = (v > best) | torch.isnan(v)
                    best, win = torch.where(take, v, best), torch.where(take, code, win)
    return best, win


def signbits(x, d):
    """The sign-bit bytes of the strided 3x3 pools' forward, (B, C, Ti, Hi/2, Wi/4) int64: bit i*4 + j of byte (a, m) is
    x[row 2a+i][column 4m+j] > 0 (a NaN is not > 0)."""
    B, C = x.shape[:2]
    pos = (x.double() > 0).to(torch.int64).reshape(B, C, d["Ti"], d["Hi"] // 2, 2, d["Wi"] // 4, 4)
    out = torch.zeros((B, C, d["Ti"], d["Hi"] // 2, d["Wi"] // 4), dtype=torch.int64, device=x.device)
    for i in range(2):
        for j in range(4):
            out |= pos[:, :, :, :, i, :, j] << (i * 4 + j)
    return out


def signbits_mask(bits, d):
    """The (B,C,Ti,Hi,Wi) boolean mask the sign-bit bytes encode."""
    B, C = bits.shape[:2]
    m = torch.zeros((B, C, d["Ti"], d["Hi"] // 2, 2, d["Wi"] // 4, 4), dtype=torch.bool, device=bits.device)
    for i in range(2):
        for j in range(4):
            m[:, :, :, :, i, :, j] = ((bits >> (i * 4 + j)) & 1) == 1
    return m.reshape(B, C, d["Ti"], d["Hi"], d["Wi"])


def pool_bwd(dy, win, d, mask=None, scale=None, old=None):
    """(dx float64 (B,C,Ti,Hi,Wi), e, K): the float64 sum of dy over the windows whose winner byte names the element (padding
    winners and halo cells drop theirs), then mask (bool; True -> * scale[c], False -> exactly 0), then + old.  e: the sum of
    the absolute terms, K: their number (the kernels add per stage, in tap order: error <= K * 2^-24 * e before the store)."""
    dy = dy.double()
    ad, one = dy.abs(), torch.ones_like(dy)
    B, C = dy.shape[:2]
    if staged(d):
        P, Ti = d["Hi"], d["Ti"]
        kt_, kh_, kw_ = (win >> 4) & 3, (win >> 2) & 3, win & 3
        outs = []
        for src in (dy, ad, one):
            gp = torch.zeros((B, C, Ti + 2, P, P), dtype=torch.float64, device=dy.device)
            for j in range(3):
                gp[:, :, j:j + Ti] += torch.where(kt_ == j, src, 0.0)
            gp = gp[:, :, 1:Ti + 1]                                             # gradients of the halo planes are dropped
            gr = torch.zeros((B, C, Ti, P + 2, P), dtype=torch.float64, device=dy.device)
            for j in range(3):
                gr[:, :, :, j:j + P, :] += torch.where(kh_ == j, gp, 0.0)
            gr = gr[:, :, :, 1:P + 1, :]
            gx = torch.zeros((B, C, Ti, P, P + 2), dtype=torch.float64, device=dy.device)
            for j in range(3):
                gx[..., j:j + P] += torch.where(kw_ == j, gr, 0.0)
            outs.append(gx[..., 1:P + 1])
        acc, e, K = outs
    else:
        dummy = torch.zeros((B, C, d["Ti"], d["Hi"], d["Wi"]), dtype=torch.float64, device=dy.device)
        outs = []
        for src in (dy, ad, one):
            gp, _ = _padded(dummy, d)
            for dt in range(d["kt"]):
                for dh in range(d["kh"]):
                    for dw in range(d["kw"]):
                        _window(gp, d, dt, dh, dw).add_(torch.where(win == (dt * d["kh"] + dh) * d["kw"] + dw, src, 0.0))
            outs.append(gp[:, :, d["pt"]:d["pt"] + d["Ti"], d["ph"]:d["ph"] + d["Hi"], d["pw"]:d["pw"] + d["Wi"]])
        acc, e, K = outs
    if mask is not None:
        sc = scale.double().view(1, C, 1, 1, 1)
        acc = torch.where(mask, acc * sc, 0.0)
        e = torch.where(mask, e * sc.abs(), 0.0)
        K = K + 1
    if old is not None:
        acc = acc + old.double()
        e = e + old.double().abs()
        K = K + 1
    return acc, e, K


# ------------------------------------------------------------------------------------------------ GroupNorm + ReLU
def gn_stats(x, G, eps, lev_pairs):
    """Per (sample, group, level): float64 mean, rstd and A = mean |x| -- (B, G, nlev) each -- and x viewed (B, G, cpg, T)."""
    x = x.double()
    B, C, T = x.shape
    xg = x.view(B, G, C // G, T)
    mean, rstd, A = [], [], []
    for lo, hi in lev_pairs:
        seg = xg[..., lo:hi]
        n = seg.shape[2] * seg.shape[3]
        m = seg.sum((2, 3)) / n
        var = ((seg - m[..., None, None]) ** 2).sum((2, 3)) / n
        mean.append(m)
        rstd.append(1.0 / torch.sqrt(var + float(eps)))
        A.append(seg.abs().sum((2, 3)) / n)
    return torch.stack(mean, -1), torch.stack(rstd, -1), torch.stack(A, -1), xg


def _per_t(v, lev_pairs, T):
    """(B, G, nlev) -> (B, G, 1, T): each level's value over its positions."""
    out = torch.empty(v.shape[:2] + (1, T), dtype=torch.float64, device=v.device)
    for l, (lo, hi) in enumerate(lev_pairs):
        out[..., 0, lo:hi] = v[..., l:l + 1]
    return out


def gn_fwd(x, gamma, beta, G, eps, relu, lev_pairs):
    """y = relu(xhat * gamma + beta) in float64 with its error scale: dict(pre, y, mean, rstd, e_y, e_mean, e_rstd, K)
    (B,C,T) / (B,G,nlev).  K = the group level's element count; e_y covers the fp32 statistics (the mean's error times
    rstd, rstd's relative error, whose second-order part is (2^-24 sqrt(K) A rstd)^2) and the affine terms."""
    B, C, T = x.shape
    mean, rstd, A, xg = gn_stats(x, G, eps, lev_pairs)
    cpg = C // G
    mt, rt, At = (_per_t(v, lev_pairs, T) for v in (mean, rstd, A))
    xhat = (xg - mt) * rt
    ga, be = gamma.double().view(1, G, cpg, 1), beta.double().view(1, G, cpg, 1)
    pre = xhat * ga + be
    K = _per_t(torch.tensor([cpg * (hi - lo) for lo, hi in lev_pairs], dtype=torch.float64, device=x.device).expand(B, G, -1),
               lev_pairs, T).expand(B, G, cpg, T)
    cond = At * rt                                      # |mean| / std: how the mean's error grows into xhat
    second = U * K.sqrt() * cond ** 2
    e_y = ga.abs() * (cond + xhat.abs() * (1 + second)) + be.abs()
    y = pre.clamp_min(0) if relu else pre
    Kl = torch.tensor([cpg * (hi - lo) for lo, hi in lev_pairs], dtype=torch.float64, device=x.device)
    return dict(pre=pre.reshape(B, C, T), y=y.reshape(B, C, T), xhat=xhat, mean=mean, rstd=rstd, A=A,
                e_y=e_y.reshape(B, C, T), K=K.reshape(B, C, T), e_mean=A, e_rstd=rstd * (1 + U * Kl.sqrt() * (A * rstd) ** 2),
                K_stats=Kl.expand(B, G, -1))


def gn_bwd(dy, x, gamma, G, eps, lev_pairs, mask):
    """dx (B,C,T) and the partials (B,3,C) = {sum_t dyh * xhat, sum_t dyh, sum_t dx} in float64, dyh = dy where mask else 0
    (mask: the library forward's y > 0, or all True without ReLU), with error scales: dict(dx, e_dx, K, part, e_part, K_part).
    dy: the float64 sum of the terms (each zero beyond its own T); pass e_dy = the sum of their absolute values."""
    B, C, T = x.shape
    cpg = C // G
    mean, rstd, A, xg = gn_stats(x, G, eps, lev_pairs)
    mt, rt, At = (_per_t(v, lev_pairs, T) for v in (mean, rstd, A))
    xhat = (xg - mt) * rt
    dyv, edy = dy[0].view(B, G, cpg, T), dy[1].view(B, G, cpg, T)
    m = mask.view(B, G, cpg, T)
    dyh = torch.where(m, dyv, 0.0)
    edyh = torch.where(m, edy, 0.0)
    ga = gamma.double().view(1, G, cpg, 1)
    g = dyh * ga
    eg = edyh * ga.abs()
    dx = torch.empty_like(g)
    e_dx = torch.empty_like(g)
    Kt = torch.empty_like(g)
    for lo, hi in lev_pairs:
        n = cpg * (hi - lo)
        sl = (Ellipsis, slice(lo, hi))
        m1 = g[sl].sum((2, 3), keepdim=True) / n
        m2 = (g[sl] * xhat[sl]).sum((2, 3), keepdim=True) / n
        M1 = eg[sl].sum((2, 3), keepdim=True) / n
        M2 = (eg[sl] * xhat[sl].abs()).sum((2, 3), keepdim=True) / n
        cond = (At[sl] * rt[sl])
        xa = xhat[sl].abs() + cond                       # |xhat| and the error the fp32 mean puts into it
        dx[sl] = rt[sl] * (g[sl] - m1 - xhat[sl] * m2)
        e_dx[sl] = rt[sl] * (eg[sl] + M1 + xa * (M2 + M1 * cond) + cond * M2)
        Kt[sl] = n
    part = torch.stack([(dyh * xhat).sum(3), dyh.sum(3), dx.sum(3)], 1).reshape(B, 3, C)
    xa_all = xhat.abs() + At * rt
    e_part = torch.stack([(edyh * xa_all).sum(3), edyh.sum(3), e_dx.sum(3)], 1).reshape(B, 3, C)
    return dict(dx=dx.reshape(B, C, T), e_dx=e_dx.reshape(B, C, T), K=Kt.reshape(B, C, T), part=part, e_part=e_part,
                K_part=Kt.reshape(B, C, T).sum(2, keepdim=True).view(B, 1, C).expand(B, 3, C))


def sum_partials(partial, B, C):
    """(3, C) float64 sums over b of partial (B, 3, C), their error scale and term count."""
    p = partial.double().reshape(B, 3, C)
    return p.sum(0), p.abs().sum(0), B


# ------------------------------------------------------------------------------------------------ glue
def bf16_bits(x):
    """fp32 -> bf16 bit patterns (int64), round to nearest even on the integer bits; a NaN becomes a quiet NaN with the same
    sign (callers compare NaN outputs as 'is a NaN')."""
    u = x.float().contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    return torch.where(nan, (u >> 16) | 0x40, r)


def bf16_nan(bits):
    return ((bits & 0x7F80) == 0x7F80) & ((bits & 0x7F) != 0)


def from_bf16_bits(bits):
    """bf16 bit patterns -> the fp32 values they denote (exact)."""
    return ((bits.to(torch.int64) & 0xFFFF) << 16).to(torch.int32).view(torch.float32)


def masked_scale_copy(src, z, scale, old=None):
    """(value float64, e, K): where(z > 0, src * scale, 0) -- a SELECT: masked positions are exactly 0 (or old) whatever src
    holds -- then + old.  Without old the value is exact once rounded to fp32 (one rounding of an exact product)."""
    sc = scale.double().view(1, -1, 1, 1) if scale is not None else torch.ones((), dtype=torch.float64, device=src.device)
    prod = src.double() * sc
    on = z.double() > 0
    val = torch.where(on, prod, 0.0)
    e = torch.where(on, prod.abs(), 0.0)
    if old is None:
        return val, e, 1
    return val.float().double() + old.double(), e + old.double().abs(), 2


def merge_fwd(p0, p1, T, up):
    """(packed (B,C,T) with only [0, t0 + t0/2) defined, frame (B,C,t0*up)) in float64; each is ONE fp32 rounding of an exact
    float64 sum (or a copy), so `.float()` of it is the exact expected fp32 value."""
    B, C, t0 = p0.shape
    p0, p1 = p0.double(), p1.double()
    idx = torch.arange(t0, device=p0.device)
    lev0 = p0 + p1[:, :, idx // 2]
    packed = torch.cat([lev0, p1], 2)
    frame = lev0[:, :, torch.arange(t0 * up, device=p0.device) // up]
    return packed, frame


def merge_bwd(da, db, dframe, dnext, t0, up):
    """(dp0, dp1) float64 with their error scales and term counts: dp0[t] = da[t] + db[t] + sum_j dframe[up t + j];
    dp1[s] = da[t0+s] + db[t0+s] + dnext[s] + dp0[2s] + dp0[2s+1] (db, dnext may be None)."""
    B, C = da.shape[:2]
    t1 = t0 // 2
    z = lambda t: torch.zeros((B, C, t), dtype=torch.float64, device=da.device)
    a, b = da.double(), (db.double() if db is not None else torch.zeros_like(da, dtype=torch.float64))
    fr = dframe.double().view(B, C, t0, up)
    dp0 = a[:, :, :t0] + b[:, :, :t0] + fr.sum(3)
    e0 = a[:, :, :t0].abs() + b[:, :, :t0].abs() + fr.abs().sum(3)
    nx = dnext.double() if dnext is not None else z(t1)
    pairs = dp0.view(B, C, t1, 2).sum(3)
    dp1 = a[:, :, t0:t0 + t1] + b[:, :, t0:t0 + t1] + nx + pairs
    e1 = a[:, :, t0:t0 + t1].abs() + b[:, :, t0:t0 + t1].abs() + nx.abs() + e0.view(B, C, t1, 2).sum(3)
    return (dp0, e0, 2 + up), (dp1, e1, 3 + 2 * (2 + up))
