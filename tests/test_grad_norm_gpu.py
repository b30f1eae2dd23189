"""GPU: otal_grad_norm / otal_adam_flat_clip against the rule of opental_amd/common/grad_clip.py, and the training step with
`track_grad_norm` / `clip_grad_norm` in every launch mode (eager, ssl beside a graph, one graph, two graphs, lane graphs, two
ranks) and through the two drivers.  Reference: AFSD/thumos14/train.py:134-141,:248-250.

Tolerances are derived in grad_norm_cases.py: the norm within ONE float32 ulp of the float64 rule, the same bits on exactly
summable inputs; the coefficient the same bits as the rule applied to the launch's own norm; the clipped Adam the same bits
as otal_adam_flat_dev wherever the pre-scaled gradient can be formed exactly, else within the existing Adam test's bound."""
import ctypes
import json
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

import grad_norm_cases as GC
import test_head_kernels_gpu as HK
from opental_amd.common import grad_clip as R

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
F32 = np.float32
NULL, SHAPE = -1, -2


@pytest.fixture(scope="module")
def lib():
    from opental_amd import _lib as L
    return L.lib()


def _vp(t):
    return ctypes.c_void_p(t.data_ptr())


def _norm_launch(lib, g0, off, grad_scale, max_norm):
    """One otal_grad_norm call on a guarded copy of g0 that starts `off` floats into its buffer (4: 16-byte aligned, 5: not).
    -> float32 (norm, coef).  The workspace starts as NaN: a partial the finish read without its block having written it,
    or one written past the grid, shows."""
    n = g0.size
    g, out = HK.Out((n,), off=off, init=g0), HK.Out((2,))
    assert g.t.data_ptr() % 16 == (off * 4) % 16
    ws = torch.full((GC.GRID_CAP + 8,), float("nan"), dtype=torch.float64, device="cuda")
    rc = lib.otal_grad_norm(g.p(), n, grad_scale, max_norm, _vp(ws), out.p(), HK.stream())
    assert rc == 0
    torch.cuda.synchronize()
    g.check("g", written=True)
    assert HK.same_bits(g.np(), g0)
    out.check("out")
    blocks = min((n + 1023) // 1024, GC.GRID_CAP)
    assert bool(torch.isnan(ws[blocks:]).all()), "a partial was written past the grid"
    o = out.np()
    return F32(o[0]), F32(o[1])


def _check_norm(label, got, g0, grad_scale, max_norm, exact):
    norm, coef = got
    want, _ = R.grad_norm_reference(g0, grad_scale, max_norm)
    print(f"{label}: norm {norm!r} reference {want!r} coef {coef!r}")
    if exact:
        assert GC.same_bits(norm, want), (label, norm, want)
    assert GC.within_one_ulp(norm, want), (label, norm, want)
    assert GC.same_bits(coef, R.clip_coefficient(norm, max_norm)), (label, coef, R.clip_coefficient(norm, max_norm))


@pytest.mark.parametrize("n", GC.SIZES)
def test_grad_norm_sizes_alignments_and_scales(lib, n):
    for kind in ("randn", "exact"):
        g0 = GC.make_input(kind, n)
        base = float(R.grad_norm_reference(g0, 1.0, 0.0)[0])
        for off in (4, 5):
            for grad_scale, max_norm in ((1.0, 0.0), (0.5, 0.37 * base + 0.01), (1.0, 0.77 * base + 0.01), (0.5, 3.0 * base + 1.0), (1.0, -2.0)):
                got = _norm_launch(lib, g0, off, grad_scale, max_norm)
                _check_norm(f"{kind} n {n} off {off - 4} scale {grad_scale} max {max_norm}", got, g0, grad_scale, max_norm, kind == "exact")
                if max_norm <= 0 or max_norm > base:
                    assert got[1] == 1.0
                elif base > 0.02:
                    assert got[1] < 1.0


@pytest.mark.parametrize("kind", ["zeros", "big", "denormal", "inf", "nan"])
def test_grad_norm_special_values(lib, kind):
    for n in (5, 4 * 256 + 1, 70001):
        g0 = GC.make_input(kind, n)
        for off in (4, 5):
            for grad_scale, max_norm in ((1.0, 5.0), (0.5, 5.0), (1.0, 0.0), (1.0, 2.5e-7)):
                got = _norm_launch(lib, g0, off, grad_scale, max_norm)
                _check_norm(f"{kind} n {n} off {off - 4} scale {grad_scale} max {max_norm}", got, g0, grad_scale, max_norm,
                            kind in ("zeros", "denormal"))
                norm, coef = got
                if kind == "zeros":         # norm 0: min(1, (1 / 1e-6) * max_norm)
                    assert norm == 0.0 and (coef == 1.0 if max_norm != 2.5e-7 else 0.2 < coef < 0.3)
                elif kind == "big":         # the square overflows float32, not float64
                    assert np.isfinite(norm) and norm > 4e17
                elif kind == "denormal":
                    assert 0.0 < norm < 2.0 ** -126
                elif kind == "inf":
                    assert np.isinf(norm) and norm > 0 and (coef == 0.0 if max_norm > 0 else coef == 1.0)
                else:
                    assert np.isnan(norm) and (np.isnan(coef) if max_norm > 0 else coef == 1.0)


def test_grad_norm_is_deterministic(lib):
    g0 = GC.make_input("randn", GC.SIZES[-1], seed=11)
    runs = [_norm_launch(lib, g0, 4, 0.5, 7.0) for _ in range(2)]
    assert GC.same_bits(runs[0][0], runs[1][0]) and GC.same_bits(runs[0][1], runs[1][1])


def test_grad_norm_refuses_bad_arguments_without_a_launch(lib):
    g, out = HK.Out((8,), init=np.ones(8, dtype=F32)), HK.Out((2,))
    ws = torch.full((GC.GRID_CAP,), float("nan"), dtype=torch.float64, device="cuda")
    assert lib.otal_grad_norm(None, 8, 1.0, 1.0, _vp(ws), out.p(), HK.stream()) == NULL
    assert lib.otal_grad_norm(g.p(), 8, 1.0, 1.0, None, out.p(), HK.stream()) == NULL
    assert lib.otal_grad_norm(g.p(), 8, 1.0, 1.0, _vp(ws), None, HK.stream()) == NULL
    assert lib.otal_grad_norm(g.p(), 0, 1.0, 1.0, _vp(ws), out.p(), HK.stream()) == SHAPE
    assert lib.otal_grad_norm(g.p(), -1, 1.0, 1.0, _vp(ws), out.p(), HK.stream()) == SHAPE
    torch.cuda.synchronize()
    out.check("out", written=False)
    assert bool(torch.isnan(ws).all())
    from opental_amd.common import ops
    with pytest.raises(RuntimeError):
        ops.grad_norm(g.t, 1.0, 1.0, out.t, ws[:100])


# ------------------------------------------------------------------------------------------------ otal_adam_flat_clip
HYPER = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=1e-3, step=7)


def _adam_launch(lib, arrays, offs, grad_scale, coef=None):
    """otal_adam_flat_clip (coef given: norm_coef = {123, coef}) or otal_adam_flat_dev on guarded copies -> float32 (p, m, v)."""
    from oracle import head_ref as H
    n = arrays[0].size
    h = HYPER
    bufs = [HK.Out((n,), off=o, init=a) for o, a in zip(offs, arrays)]
    bc = HK.dev(np.asarray(H.adam_bias_corrections(h["b1"], h["b2"], h["step"]), dtype=F32))
    p, g, m, v = bufs
    if coef is None:
        rc = lib.otal_adam_flat_dev(p.p(), g.p(), m.p(), v.p(), n, h["lr"], h["b1"], h["b2"], h["eps"], h["wd"], _vp(bc),
                                    grad_scale, HK.stream())
    else:
        nc = HK.dev(np.asarray([123.0, coef], dtype=F32))
        rc = lib.otal_adam_flat_clip(p.p(), g.p(), m.p(), v.p(), n, h["lr"], h["b1"], h["b2"], h["eps"], h["wd"], _vp(bc),
                                     grad_scale, _vp(nc), HK.stream())
    assert rc == 0
    torch.cuda.synchronize()
    for t, name in zip(bufs, "pgmv"):
        t.check(f"adam {name}")
    assert HK.same_bits(g.np(), arrays[1])
    return p.np(), m.np(), v.np()


@pytest.mark.parametrize("offs", [(4, 4, 4, 4), (4, 5, 4, 4), (5, 4, 4, 4)], ids=["aligned", "g+1", "p+1"])
@pytest.mark.parametrize("n", GC.SIZES)
def test_adam_flat_clip(lib, n, offs):
    from oracle import head_ref as H
    arrays = GC.adam_state(n)
    p0, g0, m0, v0 = arrays
    h = HYPER
    # coefficient 1: the bits of otal_adam_flat_dev
    want = _adam_launch(lib, arrays, offs, 0.5)
    got = _adam_launch(lib, arrays, offs, 0.5, coef=1.0)
    for a, b, name in zip(got, want, "pmv"):
        assert HK.same_bits(a, b), f"n {n} {offs}: coef 1 changes {name}"
    # grad_scale 1, a coefficient in (0, 1): otal_adam_flat_dev on g * coef (torch's float32 product; g * 1 is exact)
    coef = F32(0.37)
    scaled = (HK.dev(g0) * float(coef)).cpu().numpy()
    assert HK.same_bits(scaled, R.prescale(g0, 1.0, coef))
    want = _adam_launch(lib, (p0, scaled, m0, v0), offs, 1.0)
    got = _adam_launch(lib, arrays, offs, 1.0, coef=float(coef))
    for a, b, name in zip(got, want, "pmv"):
        assert HK.same_bits(a, b), f"n {n} {offs}: clipped {name} differs from the update on g * coef"
    # grad_scale 0.5: the float64 statement of the pre-scaled form, within the existing Adam test's per-element bound
    got = _adam_launch(lib, arrays, offs, 0.5, coef=float(coef))
    bc = H.adam_bias_corrections(h["b1"], h["b2"], h["step"])
    ref = R.adam_clip_reference(H.adam, p0, g0, m0, v0, 0.5, coef, lr=h["lr"], beta1=h["b1"], beta2=h["b2"], eps=h["eps"],
                                weight_decay=h["wd"], step=h["step"], bias_corr=bc)
    for a, (r, e), name in zip(got, ref, "pmv"):
        HK.check_bound("adam", f"adam_flat_clip n {n} {offs} {name}", a, r, e, 1, 0)


# ------------------------------------------------------------------------------------------------ the trainer
BATCH, STEPS = 1, 3
_RUNS = {}


@pytest.fixture()
def bf16():
    from opental_amd.common import ops
    old = ops.CONV_PRECISION
    ops.CONV_PRECISION = 1
    yield
    ops.CONV_PRECISION = old


def _norm_matches(tr, max_norm, label):
    torch.cuda.synchronize()
    got = tr.last_grad_norm.cpu().numpy()
    want, _ = R.grad_norm_reference(tr.arena.grad, 1.0 / tr.world, max_norm)
    print(f"{label}: last_grad_norm {got.tolist()} reference norm {want!r}")
    assert GC.within_one_ulp(got[0], want), (label, got, want)
    assert GC.same_bits(got[1], R.clip_coefficient(F32(got[0]), max_norm)), (label, got)
    return got


def _run(mode, clip=None, track=False, check_norms=False, steps=STEPS):
    """`steps` optimisation steps on one fixed batch from the same weights -> (p, m, v, costs, norms, trainer facts)."""
    import bench
    dev = torch.device("cuda", 0)
    clips, targets, scores = bench.synth_batch(BATCH, 1000, dev)
    tr = bench.build_trainer(dev, seed=5)
    tr.lr = 1e-4
    tr.clip_grad_norm, tr.track_grad_norm = clip, track
    done = 0
    if mode != "eager":
        tr.capture_step(clips, targets, scores, warmup=1, lanes=mode == "lanes")        # the warm-up step is a real step
        done = 1
    costs, norms = [], []
    for k in range(done, steps):
        costs.append(float(tr.step(clips, targets, scores)[0]))
        if check_norms:
            norms.append(_norm_matches(tr, clip, f"{mode} step {k + 1}"))
    torch.cuda.synchronize()
    assert tr.step_count == steps
    facts = dict(kind=None if tr._graph is None else (tr._graph[0] if isinstance(tr._graph[0], str) else "graph"),
                 replayed=tr.replayed_steps, adam_left=getattr(tr, "_adam_left", None), skipped=list(tr._skipped),
                 has_norm=tr.last_grad_norm is not None)
    a = tr.arena
    return a.flat.detach().clone(), a.m.detach().clone(), a.v.detach().clone(), costs, norms, facts


def _plain():
    if "plain" not in _RUNS:
        _RUNS["plain"] = _run("eager")
        assert not _RUNS["plain"][5]["has_norm"]        # no flag: no launch, no buffer
    return _RUNS["plain"]


def _same_run(a, b, label):
    for x, y, name in zip(a[:3], b[:3], ("p", "m", "v")):
        assert torch.equal(x, y), f"{label}: {name} differs by {float((x - y).abs().max())}"
    assert a[3][-len(b[3]):] == b[3], (label, a[3], b[3])


@pytest.mark.parametrize("mode", ["eager", "lanes"])
def test_tracking_changes_nothing_and_reports_the_norm_of_each_step(bf16, mode):
    run = _run(mode, track=True, check_norms=True)
    _same_run(_plain(), run, f"tracking, {mode}")
    assert all(n[1] == 1.0 and np.isfinite(n[0]) and n[0] > 0 for n in run[4]) and len(run[4]) == (3 if mode == "eager" else 2)
    if mode == "eager":
        _RUNS["first_norm"] = float(run[4][0][0])
    else:
        assert run[5]["kind"] == "lanes" and run[5]["replayed"] == 2


@pytest.mark.parametrize("mode", ["eager", "graph", "lanes"])
def test_a_clip_value_never_reached_leaves_the_run_as_it_was(bf16, mode):
    run = _run(mode, clip=1e30)
    _same_run(_plain(), run, f"clip 1e30, {mode}")
    assert run[5]["has_norm"] and run[5]["kind"] == (None if mode == "eager" else mode)


def _first_norm():
    if "first_norm" not in _RUNS:
        _RUNS["first_norm"] = float(_run("eager", track=True, check_norms=True, steps=1)[4][0][0])
    return _RUNS["first_norm"]


def test_one_clipped_eager_step_is_adam_on_the_scaled_gradient(bf16):
    """max_norm = half the first step's measured norm (read from a tracking run): p, m, v after the step are the saved
    p, m, v updated by otal_adam_flat_dev on arena.grad * coef."""
    import bench
    from opental_amd.common import ops
    dev = torch.device("cuda", 0)
    max_norm = 0.5 * _first_norm()
    clips, targets, scores = bench.synth_batch(BATCH, 1000, dev)
    tr = bench.build_trainer(dev, seed=5)
    tr.lr = 1e-4
    tr.clip_grad_norm = max_norm
    a = tr.arena
    p, m, v = a.flat.detach().clone(), a.m.detach().clone(), a.v.detach().clone()
    tr.step(clips, targets, scores)
    norm, coef = _norm_matches(tr, max_norm, "clipped eager step")
    assert GC.within_one_ulp(norm, F32(_first_norm())) and 0.49 < coef < 0.51 and not tr._skipped
    g = a.grad * tr.last_grad_norm[1]
    bc = torch.tensor(ops.adam_bias_corrections(1, *tr.betas), dtype=torch.float32, device=dev)
    for lo, hi, g_lr in tr._group_ranges:
        g_lr = g_lr * (tr.lr / tr._base_lr) if tr._base_lr else g_lr
        ops.adam_flat_dev(p[lo:hi], g[lo:hi], m[lo:hi], v[lo:hi], bc, g_lr, tr.betas[0], tr.betas[1], tr.eps, tr.wd, grad_scale=1.0)
    torch.cuda.synchronize()
    assert torch.equal(p, a.flat) and torch.equal(m, a.m) and torch.equal(v, a.v)


@pytest.mark.parametrize("mode", ["graph", "lanes"])
def test_clipped_trajectory_is_the_same_in_every_launch_mode(bf16, mode):
    max_norm = 0.5 * _first_norm()
    if "clip_eager" not in _RUNS:
        _RUNS["clip_eager"] = _run("eager", clip=max_norm, check_norms=True)
        assert _RUNS["clip_eager"][4][0][1] < 1.0                       # the clip really acted
        assert not torch.equal(_RUNS["clip_eager"][0], _plain()[0])
    run = _run(mode, clip=max_norm, check_norms=True)
    _same_run(_RUNS["clip_eager"], run, f"clip {max_norm}, {mode}")
    for a, b in zip(_RUNS["clip_eager"][4][-2:], run[4]):
        assert GC.same_bits(a, b)
    if mode == "lanes":
        # the lane graphs replayed, and the early Adam (everything but the stem tail, before the tail's gradients exist) was not taken
        assert run[5]["kind"] == "lanes" and run[5]["replayed"] == 2 and run[5]["adam_left"] is None


SPLIT_CODE = textwrap.dedent('''
    import os, sys, torch
    import torch.distributed as dist
    sys.path.insert(0, os.getcwd())
    sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
    import bench
    import grad_norm_cases as GC
    from opental_amd.common import grad_clip as R
    from opental_amd.common import ops
    ops.CONV_PRECISION = 1
    dev = torch.device("cuda", 0)
    dist.init_process_group(backend="nccl", device_id=dev)
    clips, targets, scores = bench.synth_batch(1, 1000, dev)
    def run(mode, clip, steps=3):
        tr = bench.build_trainer(dev, seed=5, force_collectives=True)
        tr.lr = 1e-4
        tr.net.backbone._model.split_backward = True
        tr.clip_grad_norm, tr.track_grad_norm = clip, clip is None
        done = 0
        if mode == "split":
            tr.capture_step(clips, targets, scores, warmup=1, split=True)
            assert tr._graph[0] == "split"
            done = 1
        norms = []
        for _ in range(steps - done):
            tr.step(clips, targets, scores)
            torch.cuda.synchronize()
            got = tr.last_grad_norm.cpu().numpy()
            want, _ = R.grad_norm_reference(tr.arena.grad, 1.0, clip)
            assert GC.within_one_ulp(got[0], want) and GC.same_bits(got[1], R.clip_coefficient(got[0], clip)), (mode, got, want)
            norms.append(got)
        return tr.arena.flat.detach().clone(), tr.arena.m.detach().clone(), tr.arena.v.detach().clone(), norms
    first = float(run("eager", None, steps=1)[3][0][0])
    pe, me, ve, ne = run("eager", 0.5 * first)
    ps, ms, vs, ns = run("split", 0.5 * first)
    assert ne[0][1] < 1.0, ne
    assert torch.equal(pe, ps) and torch.equal(me, ms) and torch.equal(ve, vs), float((pe - ps).abs().max())
    assert all(GC.same_bits(a, b) for a, b in zip(ne[-2:], ns)), (ne, ns)
    print("OK", first, [n.tolist() for n in ns])
    dist.destroy_process_group()
''')


def test_clipped_two_graph_step_equals_eager_steps_on_one_rccl_rank():
    """capture_step(split=True) with clipping: the norm launch and the clipped Adam run eagerly behind the second graph and
    the stem's all-reduces; the trajectory is that of eager steps in the backbone's two-node form.  (Child process, one
    forced RCCL rank: the two-graph step is the data-parallel one, and a process group is global state.)"""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29611", RANK="0", WORLD_SIZE="1",
               HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    r = subprocess.run([sys.executable, "-c", SPLIT_CODE], cwd=REPO, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "OK" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


def test_ssl_step_beside_the_lane_graphs_is_clipped_and_the_next_step_replays(bf16):
    import bench
    dev = torch.device("cuda", 0)
    max_norm = 0.05 * _first_norm()             # (far enough below that the third step's smaller gradient is clipped too)
    clips, targets, scores = bench.synth_batch(BATCH, 1000, dev)
    ssl_clips, _, _ = bench.synth_batch(BATCH, 2000, dev)
    ssl_targets = [torch.tensor([[0.30, 0.55], [0.32, 0.52], [0.70, 0.90]], device=dev) * 256 for _ in range(BATCH)]
    tr = bench.build_trainer(dev, seed=5)
    tr.lr = 1e-4
    tr.clip_grad_norm = max_norm
    tr.capture_step(clips, targets, scores, warmup=1, lanes=True)
    tr.step(clips, targets, scores)
    assert tr.replayed_steps == 1
    _norm_matches(tr, max_norm, "replayed step")
    before = tr.arena.flat.detach().clone()
    tr.step(clips, targets, scores, ssl_clips, ssl_targets)             # eager, beside the captured graphs
    assert tr.replayed_steps == 1 and tr.step_count == 3
    norm, coef = _norm_matches(tr, max_norm, "ssl step")
    assert coef < 1.0 and not torch.equal(before, tr.arena.flat)
    tr.step(clips, targets, scores)
    assert tr.replayed_steps == 2 and tr.step_count == 4 and tr._graph[0] == "lanes"
    _norm_matches(tr, max_norm, "replayed step after the ssl step")


RANK_CODE = textwrap.dedent('''
    import os, sys, torch
    import torch.distributed as dist
    sys.path.insert(0, os.getcwd())
    import bench
    from opental_amd.common import ops
    ops.CONV_PRECISION = 1
    rank, world, out = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"]), sys.argv[1]
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    dist.init_process_group(backend="gloo", rank=rank, world_size=world)
    tr = bench.build_trainer(dev, seed=5)
    assert tr.collectives and tr.world == world
    tr.lr = 1e-4
    clips, targets, scores = bench.synth_batch(1, 1000 + rank, dev)
    tr.track_grad_norm = True
    tr.step(clips, targets, scores)                     # a tracking-only eager step: the clip value is a 20th of ITS norm
    max_norm = 0.05 * float(tr.last_grad_norm[0])       # (the third step's is smaller), read on both ranks from identical bytes
    tr.clip_grad_norm, tr.track_grad_norm = max_norm, False
    tr.capture_step(clips, targets, scores, warmup=1, lanes=True)       # (the warm-up step is a real, clipped step)
    assert tr._graph[0] == "lanes"
    tr.step(clips, targets, scores)
    torch.cuda.synchronize()
    assert tr.step_count == 3 and tr.replayed_steps == 1
    torch.save({"flat": tr.arena.flat.cpu(), "m": tr.arena.m.cpu(), "grad": tr.arena.grad.cpu(), "norm": tr.last_grad_norm.cpu(),
                "max_norm": max_norm}, out + f".{rank}")
    dist.barrier()
    dist.destroy_process_group()
''')


def test_two_ranks_clip_by_the_norm_of_the_averaged_gradient(tmp_path):
    """Two rank processes on cuda:0 with gloo collectives (tests/test_dp_two_ranks_gpu.py's arrangement), clipping under
    lanes: both ranks hold bit-identical parameters, and last_grad_norm is the reference norm of the SUMMED gradient times
    1/2 -- computed on each rank from identical bytes, with no collective of its own."""
    out = str(tmp_path / "res")
    procs = []
    for r in range(2):
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29623", RANK=str(r), WORLD_SIZE="2")
        procs.append(subprocess.Popen([sys.executable, "-c", RANK_CODE, out], cwd=REPO, env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    logs = []
    for p in procs:
        try:
            o, e = p.communicate(timeout=600)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise AssertionError("the ranks did not finish")
        logs.append((p.returncode, o[-1500:], e[-3000:]))
    assert all(rc == 0 for rc, _, _ in logs), logs
    res = [torch.load(out + f".{r}") for r in range(2)]
    assert torch.equal(res[0]["flat"], res[1]["flat"]) and torch.equal(res[0]["m"], res[1]["m"])
    assert torch.equal(res[0]["grad"], res[1]["grad"]) and torch.equal(res[0]["norm"], res[1]["norm"])
    assert res[0]["max_norm"] == res[1]["max_norm"] > 0
    max_norm = res[0]["max_norm"]
    want, _ = R.grad_norm_reference(res[0]["grad"], 0.5, max_norm)
    got = res[0]["norm"].numpy()
    print("two ranks: last_grad_norm", got.tolist(), "reference", want)
    assert GC.within_one_ulp(got[0], want) and GC.same_bits(got[1], R.clip_coefficient(got[0], max_norm))
    assert got[1] < 1.0                                                 # (the clip acted: the coefficient is not the trivial one)


# ------------------------------------------------------------------------------------------------ the drivers
OLD_KEYS = {'step', 'Train/Total', 'Train/loc', 'Train/conf', 'Train/prop_loc', 'Train/prop_conf', 'Train/IoU', 'Train/start',
            'Train/end'}


def _lines(ckpt):
    return [json.loads(l) for l in open(os.path.join(ckpt, "training", "scalars.jsonl")).read().splitlines()]


def test_thumos_driver_logs_the_norm_with_the_flag_and_only_with_it(tmp_path, bf16, capsys):
    from make_synthetic_thumos import make
    from opental_amd.thumos14 import train as T
    yaml_path = make(str(tmp_path / "data"), videos=1, frames=400, size=100)
    common = [yaml_path, '--open_set', '--split', '0', '--lw', '1', '--cw', '10', '--piou', '0.5', '--ssl', '0.001', '--batch_size', '2',
              '--random_init', '--max_steps', '3', '--max_epoch', '1', '--log_every', '1']
    tr, hist = T.main(common + ['--clip_grad_norm', '5', '--checkpoint_path', str(tmp_path / "clip")])
    assert tr.clip_grad_norm == 5.0 and tr.track_grad_norm and len(hist) == 1 and len(hist[0]) == 8
    recs = _lines(str(tmp_path / "clip"))
    assert len(recs) == tr.step_count >= 1
    for r in recs:
        assert set(r) == OLD_KEYS | {'stats/grad_norm'} and np.isfinite(r['stats/grad_norm']) and r['stats/grad_norm'] > 0
    assert "grad_norm " in capsys.readouterr().out
    tr, _ = T.main(common + ['--checkpoint_path', str(tmp_path / "plain")])
    assert tr.clip_grad_norm is None and not tr.track_grad_norm and tr.last_grad_norm is None
    recs = _lines(str(tmp_path / "plain"))
    assert len(recs) == tr.step_count and all(set(r) == OLD_KEYS for r in recs)
    assert "grad_norm" not in capsys.readouterr().out


def test_anet_driver_logs_the_norm_with_the_flag_and_only_with_it(tmp_path, bf16):
    from make_synthetic_anet import make
    from opental_amd.anet import train as A
    yaml_path = make(str(tmp_path / "data"), videos=2, size=100)
    common = [yaml_path, '--open_set', '--split', '0', '--lw', '1', '--cw', '1', '--piou', '0.6', '--batch_size', '1',
              '--random_init', '--max_steps', '3', '--max_epoch', '1', '--log_every', '1']
    tr, _ = A.main(common + ['--log_grad_norm', '--checkpoint_path', str(tmp_path / "norm")])
    assert tr.clip_grad_norm is None and tr.track_grad_norm
    recs = _lines(str(tmp_path / "norm"))
    assert len(recs) == tr.step_count >= 1
    assert all(set(r) == OLD_KEYS | {'stats/grad_norm'} and r['stats/grad_norm'] > 0 for r in recs)
    tr, _ = A.main(common + ['--checkpoint_path', str(tmp_path / "plain")])
    recs = _lines(str(tmp_path / "plain"))
    assert len(recs) == tr.step_count and all(set(r) == OLD_KEYS for r in recs)
