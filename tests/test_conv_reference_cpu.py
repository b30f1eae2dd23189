"""CPU: the float64 convolution reference (oracle/conv_ref.py) that tests/test_conv_calls_gpu.py holds every recorded launch
to, checked against torch.nn.functional.conv3d in float64 (autograd for the two gradients) on small shapes: every kernel
size and stride the model records, level packing, channel slices of concat buffers, the forward epilogue, the
data-gradient mask and accumulate.  The error scale e and term count K are checked the same way, as the convolution of the
squared operands and of all-ones operands."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle.conv_ref import conv_ref, output_offsets

D = torch.float64


def same(size, k, s):
    total = (k - s) if size % s == 0 else (k - size % s)
    total = max(total, 0)
    return total // 2, (size + total - k) // s + 1


def make_geom(B, Cin, Cout, thw, k, s, valid=False, levels=None):
    pads, outs = [], []
    for size, kk, ss in zip(thw, k, s):
        p, o = (0, size - kk + 1) if (valid and kk == size) else same(size, kk, ss)
        pads.append(p)
        outs.append(o)
    nlev = len(levels) - 1 if levels else 1
    lev = list(levels) if levels else [0, thw[0]]
    lev = (lev + [0] * 9)[:9]
    return [B, Cin, Cout, *thw, *outs, *k, *s, *pads, nlev, *lev]


def torch_conv(x, w, g):
    """SAME-padded (front pads pt/ph/pw) float64 conv3d of x (B, Cin, T, H, W); levels: one conv per level."""
    B, Cin, Cout, Ti, Hi, Wi, To, Ho, Wo, kt, kh, kw, st, sh, sw, pt, ph, pw, nlev = g[:19]
    if nlev > 1:
        lev = g[19:19 + nlev + 1]
        gl = list(g)
        outs = []
        for j in range(nlev):
            n = lev[j + 1] - lev[j]
            gl[3], gl[6], gl[15], gl[18] = n, n, same(n, kt, st)[0], 1
            outs.append(torch_conv(x[:, :, lev[j]:lev[j + 1]], w, gl))
        return torch.cat(outs, 2)
    back = [(o - 1) * s + k - i - p for o, s, k, i, p in ((To, st, kt, Ti, pt), (Ho, sh, kh, Hi, ph), (Wo, sw, kw, Wi, pw))]
    xp = F.pad(x, (pw, back[2], ph, back[1], pt, back[0]))
    return F.conv3d(xp, w, stride=(st, sh, sw))


CASES = {   # name: (B, Cin, Cout, (T, H, W), k, s, spatial_valid, levels)
    "conv1a_7x7x7_s2": (2, 3, 5, (10, 12, 11), (7, 7, 7), (2, 2, 2), False, None),
    "3x3x3": (2, 6, 7, (5, 6, 7), (3, 3, 3), (1, 1, 1), False, None),
    "1x1x1": (2, 9, 4, (3, 5, 4), (1, 1, 1), (1, 1, 1), False, None),
    "3x1x1": (2, 5, 6, (6, 3, 3), (3, 1, 1), (1, 1, 1), False, None),
    "proj_1x6x6": (2, 7, 5, (4, 6, 6), (1, 6, 6), (1, 1, 1), True, None),
    "proj_1x3x3": (2, 8, 3, (5, 3, 3), (1, 3, 3), (1, 1, 1), True, None),
    "pool_3x3x3_s2": (2, 4, 3, (7, 6, 5), (3, 3, 3), (2, 2, 2), False, None),
    "1d_k1": (3, 6, 5, (9, 1, 1), (1, 1, 1), (1, 1, 1), False, None),
    "1d_k3": (3, 6, 5, (9, 1, 1), (3, 1, 1), (1, 1, 1), False, None),
    "1d_k3_s2": (2, 6, 5, (8, 1, 1), (3, 1, 1), (2, 1, 1), False, None),
    "1d_k3_levels": (2, 5, 4, (15, 1, 1), (3, 1, 1), (1, 1, 1), False, (0, 8, 12, 14, 15)),
}


def setup(name, seed=0, pad_c=(2, 3)):
    """Geometry, strides and operands of a case; x, dy and the mask are channel slices of larger concat buffers."""
    B, Cin, Cout, thw, k, s, valid, levels = CASES[name]
    g = make_geom(B, Cin, Cout, thw, k, s, valid, levels)
    To, Ho, Wo = g[6:9]
    Pi, Po = thw[0] * thw[1] * thw[2], To * Ho * Wo
    gen = torch.Generator().manual_seed(seed)
    xc, yc = Cin + sum(pad_c), Cout + sum(pad_c)
    xbuf = torch.randn(B, xc, *thw, generator=gen, dtype=D)
    ybuf = torch.randn(B, yc, To, Ho, Wo, generator=gen, dtype=D)
    mbuf = torch.randn(B, xc, *thw, generator=gen, dtype=D)
    w = torch.randn(Cout, Cin, *k, generator=gen, dtype=D)
    c0 = pad_c[0]
    strides = (xc * Pi, Pi, yc * Po, Po)
    flat = lambda t, P: t.reshape(-1)[c0 * P:]
    x, dy, m = xbuf[:, c0:c0 + Cin], ybuf[:, c0:c0 + Cout], mbuf[:, c0:c0 + Cin]
    return g, strides, w, x, dy, m, flat(xbuf, Pi), flat(ybuf, Po), flat(mbuf, Pi)


def grads(x, w, dy, g):
    x = x.clone().requires_grad_(True)
    w = w.clone().requires_grad_(True)
    y = torch_conv(x, w, g)
    gx, gw = torch.autograd.grad(y, (x, w), dy)
    return y.detach(), gx, gw


def full(mode, g):
    B, Cin, Cout, Ti, Hi, Wi, To, Ho, Wo, kt, kh, kw = g[:12]
    M = (Cout, Cin, Cout)[mode]
    N = (B * To * Ho * Wo, B * Ti * Hi * Wi, Cin * kt * kh * kw)[mode]
    return torch.arange(M), torch.arange(N)


def as_gemm(t, mode):
    """(B, C, T, H, W) output / (Cout, Cin, k..) weight gradient -> rows x cols of conv_ref."""
    if mode == 2:
        return t.reshape(t.shape[0], -1)
    return t.transpose(0, 1).reshape(t.shape[1], -1)


def close(got, want, tol=1e-12):
    scale = want.abs().max().item()
    assert scale > 0
    err = (got - want).abs().max().item()
    assert err <= tol * scale, (err, scale)


@pytest.mark.parametrize("name", sorted(CASES))
def test_forward_matches_conv3d(name):
    g, st, w, x, dy, m, xf, yf, mf = setup(name)
    gen = torch.Generator().manual_seed(1)
    scale, shift = torch.rand(g[2], generator=gen, dtype=D) + 0.5, torch.randn(g[2], generator=gen, dtype=D)
    rows, cols = full(0, g)
    y = torch_conv(x, w, g)
    for relu in (False, True):
        val, e, K = conv_ref(g, st, 0, rows, cols, x=xf, w=w, scale=scale, shift=shift, relu=relu)
        want = scale[:, None] * as_gemm(y, 0) + shift[:, None]
        close(val, want.clamp_min(0) if relu else want)
    val, e, K = conv_ref(g, st, 0, rows, cols, x=xf, w=w)
    close(val, as_gemm(y, 0))
    close(e * e, as_gemm(torch_conv(x * x, w * w, g), 0))
    close(K, as_gemm(torch_conv(torch.ones_like(x), torch.ones_like(w), g), 0), 0)


@pytest.mark.parametrize("name", sorted(CASES))
def test_data_gradient_matches_autograd(name):
    g, st, w, x, dy, m, xf, yf, mf = setup(name)
    rows, cols = full(1, g)
    _, gx, _ = grads(x, w, dy, g)
    val, e, K = conv_ref(g, st, 1, rows, cols, dy=yf, w=w)
    close(val, as_gemm(gx, 1))
    close(e * e, as_gemm(grads(x, w * w, dy * dy, g)[1], 1))
    close(K, as_gemm(grads(x, torch.ones_like(w), torch.ones_like(dy), g)[1], 1), 0)
    # the fused ReLU / BN mask and accumulate
    osc = torch.rand(g[1], dtype=D) + 0.5
    start = torch.randn(len(rows), len(cols), dtype=D)
    val, e2, _ = conv_ref(g, st, 1, rows, cols, dy=yf, w=w, mask=mf, out_scale=osc, start=start)
    keep = as_gemm((m > 0).to(D), 1) * osc[:, None]
    assert (keep == 0).any() and (keep != 0).any()
    close(val, start + keep * as_gemm(gx, 1))
    close(e2, keep * e)


@pytest.mark.parametrize("name", sorted(CASES))
def test_weight_gradient_matches_autograd(name):
    g, st, w, x, dy, m, xf, yf, mf = setup(name)
    rows, cols = full(2, g)
    _, _, gw = grads(x, w, dy, g)
    val, e, K = conv_ref(g, st, 2, rows, cols, x=xf, dy=yf, chunk=64)       # small chunks: the K loop runs several times
    close(val, as_gemm(gw, 2))
    close(e * e, as_gemm(grads(x * x, w, dy * dy, g)[2], 2))
    close(K, as_gemm(grads(torch.ones_like(x), w, torch.ones_like(dy), g)[2], 2), 0)
    start = torch.randn(len(rows), len(cols), dtype=D)
    close(conv_ref(g, st, 2, rows, cols, x=xf, dy=yf, start=start)[0], start + as_gemm(gw, 2))


def test_a_subset_is_the_same_elements_of_the_full_result():
    """Rows x cols in any order, with chunking of the columns: the elements of the full rectangle."""
    g, st, w, x, dy, m, xf, yf, mf = setup("3x3x3")
    rs = np.random.RandomState(3)
    for mode in (0, 1, 2):
        R, C = full(mode, g)
        want = conv_ref(g, st, mode, R, C, x=xf, w=w, dy=yf)[0]
        rows = torch.from_numpy(rs.permutation(len(R))[:4])
        cols = torch.from_numpy(rs.permutation(len(C))[:37])
        got = conv_ref(g, st, mode, rows, cols, x=xf, w=w, dy=yf, chunk=300)[0]
        assert torch.equal(got, want[rows][:, cols]) or (got - want[rows][:, cols]).abs().max() < 1e-12 * want.abs().max()


def test_output_offsets_address_the_output_views():
    g, st, w, x, dy, m, xf, yf, mf = setup("pool_3x3x3_s2")
    for mode, buf, view in ((0, yf, dy), (1, xf, x)):
        R, C = full(mode, g)
        off = output_offsets(g, st, mode, R, C)
        assert torch.equal(buf[off.reshape(-1)].reshape(off.shape), as_gemm(view, mode))
    R, C = full(2, g)
    assert torch.equal(output_offsets(g, st, 2, R, C).reshape(-1), torch.arange(w.numel()))
