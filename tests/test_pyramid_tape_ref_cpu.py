"""tests/pyramid_tape_ref.py, the anchored float64 reference of the detection half, checked on the CPU before anything on
a device is compared with it: it IS the oracle's restatement where nothing is anchored, its pool is the oracle's C routine,
anchoring a run on itself changes nothing -- and the anchoring is what makes an elementwise gradient check possible: a
stand-in device (an fp32 run whose 1-D convolutions sum a permuted K in two halves) meets the tolerance rule against the
anchored float64 reference and breaks it against the plain one."""
import numpy as np
import pytest
import torch

from oracle import afsd_oracle as O
from oracle import arch

import pyramid_tape_ref as R

torch.set_num_threads(min(16, torch.get_num_threads()))

CFGS = {"thumos14": (arch.THUMOS, 2), "anet": (arch.ANET, 1)}


@pytest.fixture(scope="module")
def setups():
    out = {}
    for name, (cfg, b) in CFGS.items():
        f4, f5 = R.endpoints(11, b, cfg)
        out[name] = (cfg, arch.make_params(2020, cfg), f4, f5)
    return out


@pytest.fixture(scope="module")
def plain32(setups):
    """The unanchored fp32 run of the THUMOS14 layout, its own anchor recorded."""
    cfg, pn, f4, f5 = setups["thumos14"]
    rec = {}
    run = R.Run(pn, f4, f5, cfg, torch.float32, record=rec)
    cot = R.cotangents(5, run.out, R.OUTPUTS)
    return run, rec, cot


def _oracle(pn, f4, f5, cfg):
    P = R.params(pn, torch.float32)
    a = None if f4 is None else f4.clone().requires_grad_(True)
    b = f5.clone().requires_grad_(True)
    out = O.coarse_pyramid(P, a, b, cfg)
    out["unct"] = O.dirichlet_uncertainty(out["conf"])
    out["prop_unct"] = O.dirichlet_uncertainty(out["prop_conf"])
    cot = R.cotangents(5, out, R.OUTPUTS)
    cost = sum((out[k] * cot[k]).sum() for k in R.OUTPUTS)
    names = sorted(P)
    gs = torch.autograd.grad(cost, [P[n] for n in names] + ([a] if a is not None else []) + [b])
    return out, dict(zip(names + (["input.f4"] if a is not None else []) + ["input.f5"], gs))


@pytest.mark.parametrize("name,rounding", [("thumos14", None), ("thumos14", "bf16"), ("anet", None)])
def test_unanchored_float32_reference_is_the_oracle(setups, name, rounding):
    """Every output and every gradient, bit for bit: the reference restates O.coarse_pyramid op for op (its pool picks the
    winners of oracle/bmp_ref.c, and a gather's backward adds a row's contributions in ascending proposal order, as the C
    routine does)."""
    cfg, pn, f4, f5 = setups[name]
    with O.operand_rounding(rounding):
        out_o, g_o = _oracle(pn, f4, f5, cfg)
        run = R.Run(pn, f4, f5, cfg, torch.float32)
        g_r = run.grads(R.cotangents(5, run.out, R.OUTPUTS), R.OUTPUTS)
    for k in R.OUTPUTS:
        assert torch.equal(run.out[k], out_o[k]), k
    assert set(g_r) == set(g_o)
    for n in g_o:
        assert torch.equal(g_r[n], g_o[n]), n
        assert bool(g_o[n].ne(0).any()), n


def _pool_case(rs, B, C, T, N):
    x = np.maximum(rs.standard_normal((B, C, T)), 0)                    # ties at exact zeros
    x = np.round(x * 4) / 4                                             # ... and among the positive values
    seg = rs.uniform(-0.3 * T, 1.3 * T, size=(B, N, 4))                 # windows that start or end outside [0, T)
    seg[:, ::3, 1] = seg[:, ::3, 0] - rs.uniform(0, 5, size=seg[:, ::3, 0].shape)    # inverted start windows
    seg[:, 1::4, 2] = seg[:, 1::4, 3] + 2.5                                          # inverted end windows
    seg[:, ::5] = np.round(seg[:, ::5])                                 # whole-number bounds (what proposal_windows emits)
    g = rs.randint(-8, 9, size=(B, C, N)) / 8.0                         # exactly summable in fp32, whatever the order
    return (torch.from_numpy(x.astype(np.float32)), torch.from_numpy(seg.astype(np.float32)),
            torch.from_numpy(g.astype(np.float32)))


@pytest.mark.parametrize("B,C,T,N", [(2, 8, 16, 16), (1, 6, 7, 23), (3, 4, 40, 5), (1, 2, 1, 3)])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_pool_is_the_oracles_c_routine(B, C, T, N, dtype):
    x, seg, g = _pool_case(np.random.RandomState(B * 1000 + T), B, C, T, N)
    want, want_g = O.bmp_forward(x, seg), O.bmp_backward(g, x, seg)
    assert torch.equal(want, O.bmp_forward_py(x, seg))
    xd = x.to(dtype).requires_grad_(True)
    got = R.bmp(xd, seg)
    assert got.dtype == dtype and torch.equal(got.detach().float(), want)
    (got_g,) = torch.autograd.grad((got * g.to(dtype)).sum(), xd)
    assert torch.equal(got_g.float(), want_g)
    assert bool((want_g != 0).any())
    zero = torch.zeros_like(x)                                          # an all-tie map: the first position of the window wins
    l = seg[:, :, 0].trunc().clamp(0, T - 1).long()[:, None, :].expand(B, C // 2, N)
    assert torch.equal(R.bmp_index(zero, seg)[:, :C // 2], l)


def test_self_anchored_float32_run_is_unchanged(plain32, setups):
    cfg, pn, f4, f5 = setups["thumos14"]
    run, rec, cot = plain32
    assert len(rec["blocks"]) == 21
    again = R.Run(pn, f4, f5, cfg, torch.float32, anchor=rec)
    for k in R.OUTPUTS:
        assert torch.equal(again.out[k], run.out[k]), k
    for sub in ("all", "boundary"):
        a, b = run.grads(cot, R.SUBSETS[sub]), again.grads(cot, R.SUBSETS[sub])
        for n in a:
            assert (a[n] is None) == (b[n] is None), (sub, n)
            assert a[n] is None or torch.equal(a[n], b[n]), (sub, n)


def test_self_anchored_ssl_form(setups):
    """forward(ssl=True): three maps, towers on level 0 only -- the stride-2 levels receive no gradient."""
    cfg, pn, f4, f5 = setups["thumos14"]
    rec = {}
    run = R.Run(pn, f4, f5, cfg, torch.float32, ssl=True, record=rec)
    assert sorted(run.out) == sorted(R.SSL_OUTPUTS)
    again = R.Run(pn, f4, f5, cfg, torch.float32, anchor=rec, ssl=True)
    cot = R.cotangents(6, run.out, R.SSL_OUTPUTS)
    a, b = run.grads(cot, R.SSL_OUTPUTS), again.grads(cot, R.SSL_OUTPUTS)
    for n in a:
        assert (a[n] is None) == (b[n] is None), n
        assert a[n] is None or torch.equal(a[n], b[n]), n
        dead = any(s in n for s in ("pyramids.2", "pyramids.3", "pyramids.4", "pyramids.5", "_head", "loc_heads", "cur_point_conv",
                                    "roi_conv", "proposal_conv"))
        assert (a[n] is None) == dead, n


def test_anchoring_is_what_makes_the_elementwise_check_possible(setups):
    """The stand-in device against the anchored float64 reference meets the rule of tests/test_pyramid_tape_gpu.py on all
    tensors (measured: worst ratio 4.0 of the allowed 10, on the two-element loc_head bias); against the PLAIN float64
    reference -- whose ReLU signs, pool winners and windows are its own -- it breaks it (measured: ratios up to 3e4 on the
    pyramid levels, the towers and the endpoints)."""
    cfg, pn, f4, f5 = setups["thumos14"]
    rec = {}
    with R.swap_conv1d(R.permuted_conv1d()):
        dev = R.Run(pn, f4, f5, cfg, torch.float32, record=rec)
    cot = R.cotangents(5, dev.out, R.OUTPUTS)
    got = dev.grads(cot, R.OUTPUTS)
    ref = R.Reference(pn, f4, f5, cfg, rec)
    g64, e32 = ref.grads(cot, R.OUTPUTS)
    assert len(g64) == 106
    o64, oe32 = ref.outputs()
    R.check({k: dev.out[k] for k in R.OUTPUTS}, o64, oe32, "stand-in outputs")
    fam = R.check(got, g64, e32, "stand-in gradients, anchored float64")
    assert max(v for v, _ in fam.values()) > 0.05            # (the stand-in is not the reference: the check has something to see)
    plain = R.Run(pn, f4, f5, cfg, torch.float64)
    with pytest.raises(AssertionError):
        R.check(got, plain.grads(cot, R.OUTPUTS), e32, "stand-in gradients, plain float64")
