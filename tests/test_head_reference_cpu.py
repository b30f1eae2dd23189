"""CPU: oracle/head_ref.py (the float64 / exact references behind tests/test_head_kernels_gpu.py) pinned to torch: float64
autograd of F.conv1d per level, the torch formulation of the head tails with logits exactly at +-10, 0 and 20,
F.binary_cross_entropy with m in {0, 1}, torch.optim.Adam in float64 and the C BoundaryMaxPooling oracle."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import afsd_oracle as O
from oracle import head_ref as H

T64 = torch.float64


def near(a, b, rtol=1e-12, atol=0.0):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    scale = max(float(np.abs(b).max()), 1e-300) if b.size else 1.0
    np.testing.assert_allclose(a, b, rtol=0, atol=rtol * scale + atol)


# ------------------------------------------------------------------------------------------------ head convolutions
@pytest.mark.parametrize("B,C,N,lev", [(2, 16, 9, None), (3, 16, 12, (0, 1, 2, 4, 8, 12)), (1, 32, 8, (0, 1, 2, 3, 4, 5, 6, 7, 8))])
def test_head_convs_match_conv1d_autograd_per_level(B, C, N, lev):
    rs = np.random.RandomState(1)
    in_idx, cout, ks = (1, 0, 1, 0), (2, 3, 1, 4), (3, 1, 1, 3)
    x = [rs.randn(B, C, N).astype(np.float32) for _ in range(3)]          # input 2 has no head
    w = [rs.randn(co, C, k).astype(np.float32) for co, k in zip(cout, ks)]
    bias = [rs.randn(2).astype(np.float32), None, rs.randn(1).astype(np.float32), rs.randn(4).astype(np.float32)]
    dy = [rs.randn(B, co, N).astype(np.float32) for co in cout]
    dy[1] = None
    ys, es = H.head_convs(x, w, bias, in_idx, ks, lev)
    (dxs, edx), (dws, edw), (dbs, edb) = H.head_convs_bwd(x, w, dy, in_idx, ks, lev)
    xt = [torch.tensor(a, dtype=T64, requires_grad=True) for a in x]
    wt = [torch.tensor(a, dtype=T64, requires_grad=True) for a in w]
    bt = [None if a is None else torch.tensor(a, dtype=T64, requires_grad=True) for a in bias]
    bounds = (0, N) if lev is None else lev
    total = 0
    for h, j in enumerate(in_idx):
        y = torch.cat([F.conv1d(xt[j][:, :, a:b], wt[h], bt[h], padding=ks[h] // 2) for a, b in zip(bounds, bounds[1:])], -1)
        near(ys[h], y.detach().numpy())
        assert (es[h] >= np.abs(ys[h]) * (1 - 1e-12)).all()
        if dy[h] is not None:
            total = total + (y * torch.tensor(dy[h], dtype=T64)).sum()
    total.backward()
    for j in range(3):
        want = np.zeros(x[j].shape) if xt[j].grad is None else xt[j].grad.numpy()
        near(dxs[j], want)
        assert (edx[j] >= np.abs(dxs[j]) * (1 - 1e-12)).all()
    assert not dxs[2].any()
    for h in range(4):
        near(dws[h], np.zeros(w[h].shape) if wt[h].grad is None else wt[h].grad.numpy())
        if bt[h] is not None:
            near(dbs[h], np.zeros(cout[h]) if bt[h].grad is None else bt[h].grad.numpy())
    assert not dws[1].any() and not dbs[1].any()


# ------------------------------------------------------------------------------------------------ head tails
@pytest.mark.parametrize("mode,kind", [(2, "exp"), (3, "relu"), (4, "softplus")])
def test_uncertainty_modes_match_dirichlet_layer_at_the_edges(mode, kind):
    from opental_amd.thumos14.BDNet import DirichletLayer
    rs = np.random.RandomState(mode)
    raw = H.edge_logits(mode, (2, 5, 9), rs)
    (out,), _, (u,), _ = H.head_outputs_fwd([raw], [mode], None, (0, 9), None)
    z = torch.tensor(raw, dtype=T64).permute(0, 2, 1).contiguous().requires_grad_(True)
    ut = DirichletLayer(kind).compute_uncertainty(z)
    assert np.array_equal(out, z.detach().numpy())
    near(u, ut.detach().numpy())
    if mode == 2:
        near(u, (5 / (torch.exp(torch.clamp(z, -10, 10)) + 1).sum(-1)).detach().numpy())
    du = rs.randn(2, 9)
    do = rs.randn(2, 9, 5)
    ((ut * torch.tensor(du)).sum() + (z * torch.tensor(do)).sum()).backward()
    (draw,), _, ds, _ = H.head_outputs_bwd([raw], [out.astype(np.float32)], [u], [do], [du], [mode], None, (0, 9))
    assert ds is None
    near(draw, z.grad.permute(0, 2, 1).numpy())
    (d0,), _, _, _ = H.head_outputs_bwd([raw], [out], [u], [do], [None], [mode], None, (0, 9))
    assert np.array_equal(d0, do.transpose(0, 2, 1))


def test_clamp_gradient_is_on_the_closed_interval():
    z = torch.tensor([-10.0, 10.0], dtype=T64, requires_grad=True)
    torch.exp(torch.clamp(z, -10, 10)).sum().backward()
    assert np.array_equal(z.grad.numpy(), np.exp([-10.0, 10.0]))
    assert np.array_equal(H.dalpha(np.float32([-10, 10]), 2), np.exp([-10.0, 10.0]))
    f = np.float32
    assert not H.dalpha([np.nextafter(f(-10), f(-11)), np.nextafter(f(10), f(11))], 2).any()
    assert np.array_equal(H.dalpha(f([0, -0.0, 1e-45]), 3), [0, 0, 1])
    assert H.dalpha(np.nextafter(f(20), f(21)), 4) == 1.0 and H.dalpha(f(20), 4) < 1.0


@pytest.mark.parametrize("strides", [None, (4.0, 8.0, 16.0)])
def test_scale_exp_mode_and_dscales_match_autograd(strides):
    rs = np.random.RandomState(5)
    lev = (0, 4, 5, 11)
    raw = rs.randn(2, 2, 11).astype(np.float32)
    scales = np.float32([1.0, 0.7, 1.3])
    (out,), (e,), _, _ = H.head_outputs_fwd([raw], [1], scales, lev, strides)
    s = torch.tensor(scales, dtype=T64, requires_grad=True)
    x = torch.tensor(raw, dtype=T64, requires_grad=True)
    li = torch.tensor(H.level_index(11, lev))
    f = torch.ones(3, dtype=T64) if strides is None else torch.tensor(strides, dtype=T64)
    y = (torch.exp(s[li][None, None, :] * x) * f[li][None, None, :]).permute(0, 2, 1)
    near(out, y.detach().numpy())
    do = rs.randn(2, 11, 2)
    (y * torch.tensor(do)).sum().backward()
    (draw,), _, ds, eds = H.head_outputs_bwd([raw], [out], [None], [do], [None], [1], scales, lev)
    near(draw, x.grad.numpy())
    near(ds, s.grad.numpy())
    assert (eds >= np.abs(ds)).all()
    (dz,), _, ds0, _ = H.head_outputs_bwd([raw], [out], [None], [None], [None], [1], scales, lev)
    assert not dz.any() and not ds0.any()


# ------------------------------------------------------------------------------------------------ boundary losses
@pytest.mark.parametrize("row0,step", [(0, 1), (1, 4)])
def test_boundary_bce_matches_binary_cross_entropy_with_saturated_means(row0, step):
    rs = np.random.RandomState(7)
    B, C, T = 2, 6, 9
    x = np.abs(rs.randn(B, C, T)).astype(np.float32)
    x[:, :3, 0] = 0.0; x[:, :3, 1] = 0.0; x[:, 3:, 2] = 20.0; x[:, 3:, 3] = 20.0      # m = 0, 0 | 1, 1
    mask = rs.uniform(0, 1, (B, 3, (T - 1) * step + 2)).astype(np.float32)
    mask[:, row0, 0], mask[:, row0, step] = 0.0, 1.0
    mask[:, row0 + 1, 2 * step], mask[:, row0 + 1, 3 * step] = 0.0, 1.0
    r = H.boundary_bce(x, mask, row0, step)
    assert (r["m"][:, 0, :2] == 0).all() and (r["m"][:, 1, 2:4] == 1).all() and np.tanh(20.0) == 1.0
    xt = torch.tensor(x, dtype=T64, requires_grad=True)
    m = torch.tanh(xt).view(B, 2, C // 2, T).mean(2)
    y = torch.tensor(r["y"])
    terms = F.binary_cross_entropy(m, y, reduction="none")
    near(r["terms"], terms.detach().numpy())
    assert (r["terms"][:, 0, 0] == 0).all() and (r["terms"][:, 0, 1] == 100).all()        # m = 0 under y = 0 | 1
    assert (r["terms"][:, 1, 2] == 100).all() and (r["terms"][:, 1, 3] == 0).all()
    (F.binary_cross_entropy(m[:, 0], y[:, 0]) + F.binary_cross_entropy(m[:, 1], y[:, 1])).backward()
    near(r["dx"], xt.grad.numpy())
    assert (r["dx"][:, :3, 1] == -1.0 / H.BCE_EPS / (B * T) / 3).all()          # (0 - 1) / max(0, 1e-12f)
    assert (r["e_dx"] >= np.abs(r["dx"])).all() and np.isfinite(r["e_dx"]).all() and np.isfinite(r["e_terms"]).all()
    out, e = H.boundary_finish([r["terms"], 2 * r["terms"]], [1.0, 0.1], B)
    near(out, (terms.mean(dim=(0, 2)) * (1 + 2 * float(np.float32(0.1)))).detach().numpy())
    d32 = r["dx"].astype(np.float32)
    (sc,) = H.boundary_scale([d32], [0.1], 3.0, None)
    assert np.array_equal(sc[:, :3], d32[:, :3] * (np.float32(0.1) * np.float32(3.0))) and not sc[:, 3:].any()


# ------------------------------------------------------------------------------------------------ BoundaryMaxPooling
def test_bmp_fp32_matches_the_c_oracle():
    # the C oracle converts float -> int directly: pinned inside the int range and without NaN
    x, seg, g = H.bmp_inputs(2, 6, 33, 7, 11, nan=False, huge=2e9)
    assert torch.equal(H.bmp_fwd(x, seg), O.bmp_forward(x, seg))
    gi, e = H.bmp_bwd(g, x, seg)
    want = O.bmp_backward(g, x, seg)
    assert torch.allclose(gi, want, rtol=0, atol=1e-5) and (e >= gi.abs().double().numpy() - 1e-6).all()
    xs, ss, gs = H.bmp_inputs(1, 2, 12, 5, 12, nan=False, huge=2e9)
    assert torch.equal(H.bmp_bwd(gs, xs, ss, compat_ref_stride=True)[0], O.bmp_backward(gs, xs, ss, compat_reference_bwd=True))


def test_bmp_nan_rules_levels_and_dtypes():
    x, seg, g = H.bmp_inputs(2, 6, 33, 7, 13)
    out = H.bmp_fwd(x, seg)
    py = O.bmp_forward_py(x, seg)
    assert torch.equal(torch.isnan(out), torch.isnan(py)) and torch.equal(torch.nan_to_num(out), torch.nan_to_num(py))
    assert torch.isnan(out).any()
    assert torch.equal(out[1, :3, 0], x[1, :3].max(-1).values) and torch.equal(out[1, 3:, 0], x[1, 3:, 32])
    # two levels = two independent calls side by side
    x2, seg2, g2 = H.bmp_inputs(2, 6, 5, 4, 14)
    xa, sa = torch.cat([x, x2], 2), torch.cat([seg, seg2], 1)
    lev = H.bmp_fwd(xa, sa, (0, 33, 38), (0, 7, 11))
    assert torch.equal(torch.nan_to_num(lev), torch.nan_to_num(torch.cat([out, H.bmp_fwd(x2, seg2)], 2)))
    ga = torch.cat([g, g2], 2)
    gl, _ = H.bmp_bwd(ga, xa, sa, (0, 33, 38), (0, 7, 11))
    assert torch.equal(gl, torch.cat([H.bmp_bwd(g, x, seg)[0], H.bmp_bwd(g2, x2, seg2)[0]], 2))
    wide = torch.full((2, 16, 7), 5.0)
    into = H.bmp_fwd(x, seg, into=(wide, 4))
    assert torch.equal(torch.nan_to_num(into[:, 4:10]), torch.nan_to_num(out)) and (into[:, :4] == 5).all() and (into[:, 10:] == 5).all()
    gw = torch.zeros(2, 16, 7); gw[:, 4:10] = g
    assert torch.equal(H.bmp_bwd(gw, x, seg, c0=4)[0], H.bmp_bwd(g, x, seg)[0])
    for dt in (torch.bfloat16, torch.float16, torch.float64):
        xd, gd = x.to(dt), g.to(dt)
        od = H.bmp_fwd(xd, seg)
        assert od.dtype == dt and torch.equal(torch.nan_to_num(od.double()), torch.nan_to_num(H.bmp_fwd(xd.double(), seg)))
        gd_in, _ = H.bmp_bwd(gd, xd, seg)
        assert gd_in.dtype == dt
        if dt != torch.float64:         # fp32 staging, one rounding on store
            assert torch.equal(gd_in, H.bmp_bwd(gd.float(), xd.float(), seg)[0].to(dt))


# ------------------------------------------------------------------------------------------------ Adam
@pytest.mark.parametrize("wd", [0.0, 1e-3])
def test_adam_matches_torch_optim_adam_in_float64(wd):
    rs = np.random.RandomState(17)
    n = 50
    lr, b1, b2, eps = (float(np.float32(s)) for s in (1e-3, 0.9, 0.999, 1e-8))
    p = rs.randn(n)
    pt = torch.tensor(p, dtype=T64, requires_grad=True)
    opt = torch.optim.Adam([pt], lr=lr, betas=(b1, b2), eps=eps, weight_decay=float(np.float32(wd)))
    m, v = np.zeros(n), np.zeros(n)
    for step in range(1, 4):
        g = rs.randn(n)
        pt.grad = torch.tensor(g * 0.5, dtype=T64)
        opt.step()
        bc = (1.0 - b1 ** step, np.sqrt(1.0 - b2 ** step))           # torch keeps them in double
        (p, ep), (m, em), (v, ev) = H.adam(p, g, m, v, lr, b1, b2, eps, wd, step, grad_scale=0.5, bias_corr=bc)
        near(p, pt.detach().numpy(), rtol=1e-13)
        assert (ep >= np.abs(p)).all() and (em >= np.abs(m)).all() and (ev >= v).all()
    st = opt.state[pt]
    near(m, st["exp_avg"].numpy(), rtol=1e-13)
    near(v, st["exp_avg_sq"].numpy(), rtol=1e-13)
    c1, c2 = H.adam_bias_corrections(0.9, 0.999, 100000)
    assert c1 == np.float32(1.0) and c2 == np.float32(1.0)
    c1, c2 = H.adam_bias_corrections(0.9, 0.999, 1)
    assert c1 == np.float32(1.0 - float(np.float32(0.9))) and c2 == np.float32(np.sqrt(1.0 - float(np.float32(0.999))))
