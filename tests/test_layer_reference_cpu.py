"""CPU: the float64 / exact layer references (oracle/layer_ref.py) that tests/test_layer_calls_gpu.py holds every recorded
max-pool, GroupNorm and glue launch to, pinned to torch: F.max_pool3d over F.pad (indices mapped to winner bytes, float64
autograd for the backward), float64 autograd of oracle.afsd_oracle.gn_relu (one call per level), Tensor.to(torch.bfloat16)
and F.interpolate."""
import pytest
import torch
import torch.nn.functional as F

from oracle import afsd_oracle
from oracle import layer_ref as R

D = torch.float64


def same(size, k, s):
    total = max((k - s) if size % s == 0 else (k - size % s), 0)
    return total // 2, total - total // 2, (size + total - k) // s + 1


def geom(B, C, thw, k, s):
    pads, backs, outs = [], [], []
    for size, kk, ss in zip(thw, k, s):
        f, b, o = same(size, kk, ss)
        pads.append(f)
        backs.append(b)
        outs.append(o)
    return dict(zip(R.GEOM, [B, C, *thw, *outs, *k, *s, *pads])), backs


def tie_input(shape, gen, nan=0):
    """Values on a coarse grid (most windows hold ties), mostly negative planes (the padding wins), exact zeros, NaNs."""
    x = torch.randint(-3, 2, shape, generator=gen).to(D) * 0.5
    x[:, :, 0] = -torch.rand(shape[0], shape[1], *shape[3:], generator=gen, dtype=D) - 0.5     # negative planes: the padding wins
    x[:, :, -1] = -torch.rand(shape[0], shape[1], *shape[3:], generator=gen, dtype=D) - 0.5
    if nan:
        idx = torch.randint(0, x.numel(), (nan,), generator=gen)
        x.view(-1)[idx] = float("nan")
    return x


def torch_pool(x, d, backs):
    pads = [d["pw"], backs[2], d["ph"], backs[1], d["pt"], backs[0]]
    xp = F.pad(x, pads)
    y, idx = F.max_pool3d(xp, (d["kt"], d["kh"], d["kw"]), (d["st"], d["sh"], d["sw"]), return_indices=True)
    return xp, y, idx


def torch_winner(idx, xp_shape, d):
    """Flat indices into the padded input -> (dt, dh, dw) of each window, and whether that tap is a padded zero."""
    Tp, Hp, Wp = xp_shape[2:]
    t, r = idx // (Hp * Wp), idx % (Hp * Wp)
    h, w = r // Wp, r % Wp
    To, Ho, Wo = idx.shape[2:]
    to = torch.arange(To).view(-1, 1, 1)
    ho = torch.arange(Ho).view(1, -1, 1)
    wo = torch.arange(Wo).view(1, 1, -1)
    dt, dh, dw = t - to * d["st"], h - ho * d["sh"], w - wo * d["sw"]
    ti, hi, wi = t - d["pt"], h - d["ph"], w - d["pw"]
    pad = (ti < 0) | (ti >= d["Ti"]) | (hi < 0) | (hi >= d["Hi"]) | (wi < 0) | (wi >= d["Wi"])
    return dt, dh, dw, pad


def staged_winner(win, d):
    """(dt, dh, dw, padded) of each output that the STAGED bytes name (followed through the three stages)."""
    Ti, P = d["Ti"], d["Hi"]
    kt_, kh_, kw_ = (win >> 4) & 3, (win >> 2) & 3, win & 3
    B, C = win.shape[:2]
    t = torch.arange(Ti).view(1, 1, -1, 1, 1).expand_as(win)
    h = torch.arange(P).view(1, 1, 1, -1, 1).expand_as(win)
    w = torch.arange(P).view(1, 1, 1, 1, -1).expand_as(win)
    bb = torch.arange(B).view(-1, 1, 1, 1, 1).expand_as(win)
    cc = torch.arange(C).view(1, -1, 1, 1, 1).expand_as(win)
    dt = kt_
    tp = t + dt - 1
    pad = (tp < 0) | (tp >= Ti)
    dh = kh_[bb, cc, tp.clamp(0, Ti - 1), h, w]
    hp = h + dh - 1
    pad |= (hp < 0) | (hp >= P)
    dw = kw_[bb, cc, tp.clamp(0, Ti - 1), hp.clamp(0, P - 1), w]
    wp = w + dw - 1
    pad |= (wp < 0) | (wp >= P)
    return dt, dh, dw, pad


POOLS = [((2, 3, (4, 6, 8), (1, 3, 3), (1, 2, 2))), ((1, 2, (6, 6, 8), (3, 3, 3), (2, 2, 2))), ((1, 2, (5, 7, 9), (1, 3, 3), (1, 2, 2))),
         ((1, 2, (4, 5, 5), (2, 2, 2), (2, 2, 2))), ((1, 2, (5, 6, 7), (3, 3, 3), (1, 1, 1))), ((1, 2, (4, 5, 6), (2, 3, 1), (1, 2, 1))),
         ((1, 2, (5, 6, 6), (3, 3, 3), (1, 1, 1))), ((2, 2, (4, 3, 3), (3, 3, 3), (1, 1, 1))), ((1, 1, (3, 12, 12), (3, 3, 3), (1, 1, 1)))]


@pytest.mark.parametrize("case", POOLS, ids=[f"{c[2]}-k{c[3]}-s{c[4]}" for c in POOLS])
@pytest.mark.parametrize("nan", [0, 3])
def test_pool_forward_matches_max_pool3d(case, nan):
    B, C, thw, k, s = case
    d, backs = geom(B, C, thw, k, s)
    gen = torch.Generator().manual_seed(hash((thw, k, s, nan)) % 1000)
    x = tie_input((B, C) + thw, gen, nan)
    y, win = R.pool_fwd(x, d)
    xp, ty, idx = torch_pool(x, d, backs)
    assert torch.equal(torch.isnan(y), torch.isnan(ty))
    assert torch.equal(torch.nan_to_num(y, 7.0), torch.nan_to_num(ty, 7.0))
    dt, dh, dw, pad = torch_winner(idx, xp.shape, d)
    if R.staged(d):
        sdt, sdh, sdw, spad = staged_winner(win, d)
        assert torch.equal(spad, pad)
        assert torch.equal(torch.where(pad, 0, sdt), torch.where(pad, 0, dt))
        assert torch.equal(torch.where(pad, 0, sdh), torch.where(pad, 0, dh))
        assert torch.equal(torch.where(pad, 0, sdw), torch.where(pad, 0, dw))
    else:
        want = torch.where(pad, 255, (dt * d["kh"] + dh) * d["kw"] + dw)
        assert torch.equal(win, want)


@pytest.mark.parametrize("case", POOLS, ids=[f"{c[2]}-k{c[3]}-s{c[4]}" for c in POOLS])
def test_pool_backward_matches_autograd(case):
    B, C, thw, k, s = case
    d, backs = geom(B, C, thw, k, s)
    gen = torch.Generator().manual_seed(7)
    x = tie_input((B, C) + thw, gen).requires_grad_(True)
    xp, ty, _ = torch_pool(x, d, backs)
    dy = torch.randn(ty.shape, generator=gen, dtype=D)
    (gx,) = torch.autograd.grad(ty, x, dy)
    _, win = R.pool_fwd(x.detach(), d)
    acc, e, K = R.pool_bwd(dy, win, d)
    assert torch.allclose(acc, gx, rtol=0, atol=1e-12)
    ((gx_abs,),) = (torch.autograd.grad(torch_pool(x, d, backs)[1], x, dy.abs()),)
    assert torch.allclose(e, gx_abs, rtol=0, atol=1e-12)
    ((gk,),) = (torch.autograd.grad(torch_pool(x, d, backs)[1], x, torch.ones_like(dy)),)
    assert torch.equal(K, gk)
    # the mask selects (masked elements exactly 0 whatever the sum), the scale multiplies, old is added last
    mask = torch.rand(acc.shape, generator=gen) > 0.5
    scale = torch.rand(C, generator=gen, dtype=D) + 0.5
    old = torch.randn(acc.shape, generator=gen, dtype=D)
    v, e2, K2 = R.pool_bwd(dy, win, d, mask=mask, scale=scale, old=old)
    want = torch.where(mask, gx * scale.view(1, -1, 1, 1, 1), 0.0) + old
    assert torch.allclose(v, want, rtol=0, atol=1e-12)
    assert torch.equal(K2, K + 2)


def test_signbits_layout():
    d, _ = geom(1, 2, (2, 4, 8), (1, 3, 3), (1, 2, 2))
    x = torch.randn(1, 2, 2, 4, 8, dtype=D)
    x[0, 0, 0, 0, 0] = float("nan")
    bits = R.signbits(x, d)
    assert bits.shape == (1, 2, 2, 2, 2)
    for t in range(2):
        for a in range(2):
            for m in range(2):
                want = sum(int(bool(x[0, 1, t, 2 * a + i, 4 * m + j] > 0)) << (i * 4 + j) for i in range(2) for j in range(4))
                assert int(bits[0, 1, t, a, m]) == want
    assert torch.equal(R.signbits_mask(bits, d), x > 0)


# ------------------------------------------------------------------------------------------------ GroupNorm
def gn_torch(x, gamma, beta, lev):
    outs = [afsd_oracle.gn_relu(x[:, :, lo:hi], gamma, beta) for lo, hi in lev]
    return torch.cat(outs, 2)


@pytest.mark.parametrize("T,lev", [(37, None), (40, [0, 24, 32, 36, 38, 39, 40]), (9, [0, 3, 9])])
def test_gn_forward_and_backward_match_autograd(T, lev):
    B, C, G, eps = 2, 64, 32, 1e-5
    gen = torch.Generator().manual_seed(T)
    pairs = R.levels(T, len(lev) - 1 if lev else 1, lev)
    x = torch.randn(B, C, T, generator=gen, dtype=D) * 2 + 0.5
    x[:, :2] += 1000.0                                                      # group 0: mean >> std
    x[1, 2:4] = 3.0                                                         # a constant group
    gamma = torch.randn(C, generator=gen, dtype=D)
    beta = torch.randn(C, generator=gen, dtype=D) * 0.5
    xr = x.clone().requires_grad_(True)
    gr, br = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    y = gn_torch(xr, gr, br, pairs)
    f = R.gn_fwd(x, gamma, beta, G, eps, 1, pairs)
    assert torch.allclose(f["y"], y.detach(), rtol=1e-9, atol=1e-9)
    assert float(f["rstd"][1, 1].min()) == pytest.approx(1 / eps ** 0.5)
    terms = [torch.randn(B, C, T, generator=gen, dtype=D), torch.randn(B, C, T - 2, generator=gen, dtype=D)]
    dy = terms[0].clone()
    dy[:, :, :T - 2] += terms[1]
    gx, gg, gb = torch.autograd.grad(y, (xr, gr, br), dy)
    mask = f["y"] > 0
    b = R.gn_bwd((dy, dy.abs()), x, gamma, G, eps, pairs, mask)
    assert torch.allclose(b["dx"], gx, rtol=1e-7, atol=1e-7)
    part = b["part"].sum(0)
    assert torch.allclose(part[0], gg, rtol=1e-9, atol=1e-9)
    assert torch.allclose(part[1], gb, rtol=1e-9, atol=1e-9)
    assert torch.allclose(part[2], gx.sum((0, 2)), rtol=1e-7, atol=1e-7)
    s, e, K = R.sum_partials(b["part"], B, C)
    assert torch.allclose(s, part) and K == B and torch.all(e >= s.abs())


# ------------------------------------------------------------------------------------------------ glue
def test_bf16_conversion_matches_torch():
    special = torch.tensor([0x7F7FFFFF, 0x7F800000, 0xFF800000, 0x00000000, 0x80000000, 0x00000001, 0x007FFFFF, 0x80400000,
                            0x3F808000, 0x3F818000, 0x3F80C000, 0x3F807FFF, 0x7F7F8000, 0x7FC00000, 0xFFC00001, 0x7F800001],
                           dtype=torch.int64).to(torch.int32)
    rnd = torch.randint(-2 ** 31, 2 ** 31 - 1, (4096,), generator=torch.Generator().manual_seed(1), dtype=torch.int64).to(torch.int32)
    x = torch.cat([special, rnd]).view(torch.float32)
    got = R.bf16_bits(x)
    want = x.to(torch.bfloat16).view(torch.int16).to(torch.int64) & 0xFFFF
    nan = torch.isnan(x)
    assert torch.equal(got[~nan], want[~nan])
    assert bool(R.bf16_nan(got[nan]).all()) and bool(R.bf16_nan(want[nan]).all())
    assert int(got[0]) == 0x7F80                                           # 0x7F7FFFFF rounds up to +inf
    back = R.from_bf16_bits(want)
    assert torch.equal(back[~nan], x.to(torch.bfloat16).float()[~nan])


def test_masked_scale_copy_selects():
    gen = torch.Generator().manual_seed(3)
    src = torch.randn(2, 3, 4, 8, generator=gen)
    src[0, 0, 0, :3] = torch.tensor([float("inf"), float("nan"), -float("inf")])
    z = torch.randn(2, 3, 4, 8, generator=gen)
    z[0, 0, 0, :3] = -1.0
    scale = torch.rand(3, generator=gen) + 0.5
    v, e, K = R.masked_scale_copy(src, z, scale)
    assert torch.equal(v[0, 0, 0, :3], torch.zeros(3, dtype=D))
    assert torch.equal(v.float(), torch.where(z > 0, src * scale.view(1, -1, 1, 1), torch.zeros(())))


def test_pyramid_merge_matches_interpolate():
    gen = torch.Generator().manual_seed(5)
    B, C, t0, up = 2, 3, 8, 4
    T = t0 + t0 // 2 + 5
    p0 = torch.randn(B, C, t0, generator=gen, dtype=D).requires_grad_(True)
    p1 = torch.randn(B, C, t0 // 2, generator=gen, dtype=D).requires_grad_(True)
    lev0 = p0 + F.interpolate(p1, size=t0, mode="nearest")
    frame = F.interpolate(lev0.unsqueeze(-1), size=[t0 * up, 1], mode="nearest").squeeze(-1)
    packed, fr = R.merge_fwd(p0.detach(), p1.detach(), T, up)
    assert torch.equal(packed[:, :, :t0], lev0.detach()) and torch.equal(packed[:, :, t0:], p1.detach())
    assert torch.equal(fr, frame.detach())
    da, db = torch.randn(B, C, T, generator=gen, dtype=D), torch.randn(B, C, T, generator=gen, dtype=D)
    dframe, dnext = torch.randn(B, C, t0 * up, generator=gen, dtype=D), torch.randn(B, C, t0 // 2, generator=gen, dtype=D)
    out = (lev0 * (da[:, :, :t0] + db[:, :, :t0])).sum() + (p1 * (da[:, :, t0:t0 + t0 // 2] + db[:, :, t0:t0 + t0 // 2] + dnext)).sum() \
        + (frame * dframe).sum()
    g0, g1 = torch.autograd.grad(out, (p0, p1))
    (dp0, e0, K0), (dp1, e1, K1) = R.merge_bwd(da, db, dframe, dnext, t0, up)
    assert torch.allclose(dp0, g0, rtol=0, atol=1e-12) and torch.allclose(dp1, g1, rtol=0, atol=1e-12)
    assert K0 == 2 + up and torch.all(e0 >= dp0.abs())
