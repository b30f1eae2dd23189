"""GPU: otal_adam_flat_sched against the rule of opental_amd/common/lr_schedule.py, and the training step with `lr_schedule` /
`ema_decay` in every launch mode (eager, ssl beside the lane graphs, one graph, two graphs on one RCCL rank, lane graphs) and
through the two drivers and score_checkpoints --ema.

Tolerances are derived in lr_schedule_cases.py: p, m, v the same bits as otal_adam_flat_dev / otal_adam_flat_clip at the
float32 product of rate and multiplier; the EMA within ONE float32 ulp of the float64 rule applied to the launch's own p', the
same bits where the line is exact; the whole update within the existing Adam test's per-element bound."""
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
import lr_schedule_cases as LC
import test_head_kernels_gpu as HK
from opental_amd.common import grad_clip as R
from opental_amd.common import lr_schedule as S

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
F32 = np.float32
NULL, SHAPE = -1, -2
HYPER = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=1e-3, step=7)
SIZES = LC.sizes(GC.SIZES)
ALIGN = pytest.mark.parametrize("offs", list(LC.ALIGNMENTS.values()), ids=list(LC.ALIGNMENTS))


@pytest.fixture(scope="module")
def lib():
    from opental_amd import _lib as L
    return L.lib()


def _vp(t):
    return ctypes.c_void_p(t.data_ptr())


def _bias():
    from oracle import head_ref as H
    return np.asarray(H.adam_bias_corrections(HYPER["b1"], HYPER["b2"], HYPER["step"]), dtype=F32)


def _launch(lib, arrays, offs, grad_scale, entry="sched", mult=1.0, keep=0.0, ema=None, coef=None, lr=None, wd=None):
    """One launch on guarded copies -> float32 (p, m, v, ema or None).  entry: 'sched' (otal_adam_flat_sched; ema / coef None:
    that pointer is NULL), 'dev' (otal_adam_flat_dev) or 'clip' (otal_adam_flat_clip).  The step record sits 4 bytes past a
    16-byte boundary whenever an array does: nothing may assume its alignment."""
    n = arrays[0].size
    h = dict(HYPER, lr=HYPER["lr"] if lr is None else lr, wd=HYPER["wd"] if wd is None else wd)
    bufs = [HK.Out((n,), off=o, init=a) for o, a in zip(offs, arrays)]
    for t, o in zip(bufs, offs):
        assert t.t.data_ptr() % 16 == (o * 4) % 16
    p, g, m, v = bufs
    e = None if ema is None else HK.Out((n,), off=offs[4], init=ema)
    shift = int(any(o != 4 for o in offs))
    rec = HK.dev(np.concatenate([np.full(shift, 77.0, dtype=F32), S.step_state(_bias(), mult, keep)]))[shift:]
    assert rec.data_ptr() % 16 == 4 * shift
    nc = None if coef is None else HK.dev(np.asarray([123.0, coef], dtype=F32))
    head = (p.p(), g.p(), m.p(), v.p())
    tail = (h["lr"], h["b1"], h["b2"], h["eps"], h["wd"])
    if entry == "sched":
        rc = lib.otal_adam_flat_sched(*head, None if e is None else e.p(), n, *tail, _vp(rec), grad_scale,
                                      None if nc is None else _vp(nc), HK.stream())
    elif entry == "dev":
        rc = lib.otal_adam_flat_dev(*head, n, *tail, _vp(rec), grad_scale, HK.stream())
    else:
        rc = lib.otal_adam_flat_clip(*head, n, *tail, _vp(rec), grad_scale, _vp(nc), HK.stream())
    assert rc == 0
    torch.cuda.synchronize()
    for t, name in zip(bufs + ([e] if e is not None else []), "pgmve"):
        t.check(f"adam_flat_sched {name}")              # guard bands untouched, every element written
    assert HK.same_bits(g.np(), arrays[1])
    return p.np(), m.np(), v.np(), None if e is None else e.np()


def _same(got, want, label):
    for a, b, name in zip(got[:3], want[:3], "pmv"):
        assert HK.same_bits(a, b), f"{label}: {name} differs"


@ALIGN
@pytest.mark.parametrize("n", SIZES)
def test_multipliers_against_adam_flat_dev_and_clip(lib, n, offs):
    arrays = GC.adam_state(n)
    label = f"n {n} {offs}"
    # multiplier 1, ema NULL, norm_coef NULL: the bits of otal_adam_flat_dev
    dev = _launch(lib, arrays, offs, 0.5, entry="dev")
    one = _launch(lib, arrays, offs, 0.5)
    _same(one, dev, label + " multiplier 1")
    assert one[3] is None
    # multiplier 0.37f: otal_adam_flat_dev at the float32 product formed on the host (the rule's effective_lr32)
    lr32 = F32(HYPER["lr"]) * F32(0.37)
    assert GC.same_bits(lr32, S.effective_lr32(HYPER["lr"], 0.37))
    _same(_launch(lib, arrays, offs, 0.5, mult=0.37), _launch(lib, arrays, offs, 0.5, entry="dev", lr=float(lr32)), label + " multiplier 0.37")
    # multiplier 0: p keeps its bits, m and v are updated
    zero = _launch(lib, arrays, offs, 0.5, mult=0.0)
    assert HK.same_bits(zero[0], arrays[0]) and HK.same_bits(zero[1], dev[1]) and HK.same_bits(zero[2], dev[2])
    assert n < 3 or not HK.same_bits(zero[1], arrays[2])
    # norm_coef given: the bits of otal_adam_flat_clip, with and without a multiplier
    _same(_launch(lib, arrays, offs, 0.5, coef=0.37), _launch(lib, arrays, offs, 0.5, entry="clip", coef=0.37), label + " clip")
    _same(_launch(lib, arrays, offs, 1.0, mult=0.37, coef=0.61), _launch(lib, arrays, offs, 1.0, entry="clip", coef=0.61, lr=float(lr32)),
          label + " clip x multiplier")


@ALIGN
@pytest.mark.parametrize("n", SIZES)
def test_ema_line(lib, n, offs):
    arrays, ema0 = GC.adam_state(n), LC.ema_state(n)
    label = f"n {n} {offs}"
    plain = _launch(lib, arrays, offs, 0.5, mult=0.8)
    for clip in (None, 0.37):
        base = plain if clip is None else _launch(lib, arrays, offs, 0.5, mult=0.8, coef=clip)
        # keep = 1: ema's bits stay; p, m, v do not see the fifth array
        got = _launch(lib, arrays, offs, 0.5, mult=0.8, keep=1.0, ema=ema0, coef=clip)
        _same(got, base, label + " keep 1")
        assert HK.same_bits(got[3], ema0), label
        # keep = 0: ema takes the bits of the new p.  The line is fl(fl(p' - ema) + ema): p' itself wherever p' - ema is a
        # float32 value, which Sterbenz's lemma gives for ema within a factor two of p' -- an average that tracks the weights.
        # The launch's p' is known (p, m, v do not see the fifth array: checked above), so ema = p' * c with c in [0.6, 1.9].
        near = (base[0] * np.random.RandomState(n).uniform(0.6, 1.9, n).astype(F32)).astype(F32)
        got = _launch(lib, arrays, offs, 0.5, mult=0.8, keep=0.0, ema=near, coef=clip)
        _same(got, base, label + " keep 0")
        assert HK.same_bits(got[3], got[0]), label
        # ... and on an ema unrelated to p' (randn) it is the rule's value for keep = 0, within one ulp like every keep
        got = _launch(lib, arrays, offs, 0.5, mult=0.8, keep=0.0, ema=ema0, coef=clip)
        _same(got, base, label + " keep 0, far ema")
        dist = LC.ulp_distance(got[3], S.ema_reference(ema0, got[0], 0.0).astype(F32))
        print(f"{label} clip {clip}: keep 0 on a far ema: {int((LC.ulp_distance(got[3], got[0]) > 0).sum())} of {n} are not p' bit for bit")
        assert int(dist.max()) <= 1, label
        # keep = 0.999 on randn inputs: within one float32 ulp of the float64 rule on the launch's own p' and the old ema
        got = _launch(lib, arrays, offs, 0.5, mult=0.8, keep=0.999, ema=ema0, coef=clip)
        _same(got, base, label + " keep 0.999")
        want = S.ema_reference(ema0, got[0], 0.999)
        dist = LC.ulp_distance(got[3], want.astype(F32))
        print(f"{label} clip {clip}: ema ulp distance max {int(dist.max())}, {int((dist > 0).sum())} of {n} differ")
        assert int(dist.max()) <= 1, label
        assert n < 3 or not HK.same_bits(got[3], ema0)
    # keep = 0.5 on dyadic inputs (g = m = v = 0, no decay: p' = p; p - ema, its half and the sum are exact): the rule's bits
    p, g, m, v, e = LC.dyadic_state(n)
    got = _launch(lib, (p, g, m, v), offs, 1.0, mult=0.8, keep=0.5, ema=e, wd=0.0)
    assert HK.same_bits(got[0], p)
    want = S.ema_reference(e, p, 0.5)
    assert np.array_equal(want, e.astype(np.float64) + (p.astype(np.float64) - e.astype(np.float64)) * 0.5)     # (exact throughout)
    assert HK.same_bits(got[3], want.astype(F32)), label


@ALIGN
@pytest.mark.parametrize("n", SIZES)
def test_everything_at_once_within_the_adam_bound(lib, n, offs):
    from oracle import head_ref as H
    arrays, ema0 = GC.adam_state(n), LC.ema_state(n)
    h = HYPER
    coef, mult, keep = F32(0.37), 0.61, S.ema_keep(0.999, h["step"])
    got = _launch(lib, arrays, offs, 0.5, mult=mult, keep=float(keep), ema=ema0, coef=float(coef))
    ref = S.adam_sched_reference(H.adam, *arrays, 0.5, h["lr"], mult, coef=coef, ema=ema0, keep=keep, beta1=h["b1"], beta2=h["b2"],
                                 eps=h["eps"], weight_decay=h["wd"], step=h["step"], bias_corr=_bias())
    for a, (r, e), name in zip(got, ref, ("p", "m", "v", "ema")):
        HK.check_bound("adam", f"adam_flat_sched n {n} {offs} {name}", a, r, e, 1, 0)


def test_refuses_bad_arguments_without_a_launch(lib):
    from opental_amd.common import ops
    init = np.ones(8, dtype=F32)
    bufs = [HK.Out((8,), init=init) for _ in range(5)]
    p, g, m, v, e = bufs
    rec = HK.dev(S.step_state(_bias(), 0.5, 0.5))
    nc = HK.dev(np.asarray([1.0, 0.5], dtype=F32))
    args = (1e-3, 0.9, 0.999, 1e-8, 0.0)
    for k in range(4):
        ptrs = [None if j == k else b.p() for j, b in enumerate(bufs[:4])]
        assert lib.otal_adam_flat_sched(*ptrs, e.p(), 8, *args, _vp(rec), 1.0, _vp(nc), HK.stream()) == NULL
    assert lib.otal_adam_flat_sched(p.p(), g.p(), m.p(), v.p(), e.p(), 8, *args, None, 1.0, _vp(nc), HK.stream()) == NULL
    assert lib.otal_adam_flat_sched(p.p(), g.p(), m.p(), v.p(), e.p(), 0, *args, _vp(rec), 1.0, _vp(nc), HK.stream()) == SHAPE
    assert lib.otal_adam_flat_sched(p.p(), g.p(), m.p(), v.p(), None, -1, *args, _vp(rec), 1.0, None, HK.stream()) == SHAPE
    torch.cuda.synchronize()
    for b in bufs:
        b.check("refused")
        assert HK.same_bits(b.np(), init)
    with pytest.raises(RuntimeError):
        ops.adam_flat_sched(p.t, g.t, m.t, v.t, rec[:2], 1e-3)
    with pytest.raises(RuntimeError):
        ops.adam_flat_sched(p.t, g.t, m.t, v.t, rec, 1e-3, ema=e.t[:4])
    # the wrapper: the same launch
    ops.adam_flat_sched(p.t, g.t, m.t, v.t, rec, 1e-3, 0.9, 0.999, 1e-8, 0.0, ema=e.t, norm_coef=nc)
    torch.cuda.synchronize()
    assert not HK.same_bits(p.np(), init) and not HK.same_bits(e.np(), init)


# ------------------------------------------------------------------------------------------------ the trainer
BATCH, STEPS = 1, 3
CONSTANT = dict(name='constant', total_steps=6)
COSINE = dict(name='cosine', total_steps=6, warmup_steps=2)
_RUNS = {}


@pytest.fixture()
def bf16():
    from opental_amd.common import ops
    old = ops.CONV_PRECISION
    ops.CONV_PRECISION = 1
    yield
    ops.CONV_PRECISION = old


def _record_matches(tr, t, label):
    """The device record after step t: Adam's bias corrections, float32(multiplier(t)), ema_keep(decay, t)."""
    from opental_amd.common import ops
    got = tr._bias_corr.cpu().numpy()
    keep = 0.0 if tr.ema_decay is None else S.ema_keep(tr.ema_decay, t)
    want = S.step_state(ops.adam_bias_corrections(t, *tr.betas), tr.lr_multiplier(t), keep)
    assert got.shape == (4,) and GC.same_bits(got, want), (label, got, want)
    return float(got[2])


def _ema_matches(tr, prev, t, label):
    """arena.ema after step t against the rule on the trainer's own previous ema and current weights."""
    torch.cuda.synchronize()
    a = tr.arena
    want = S.ema_reference(prev.cpu().numpy(), a.flat.detach().cpu().numpy(), S.ema_keep(tr.ema_decay, t)).astype(F32)
    dist = LC.ulp_distance(a.ema.cpu().numpy(), want)
    print(f"{label} step {t}: ema ulp distance max {int(dist.max())}, {int((dist > 0).sum())} of {dist.size} differ")
    assert int(dist.max()) <= 1, label
    assert not torch.equal(a.ema, prev) and not torch.equal(a.ema, a.flat)


def _run(mode, schedule=None, ema=None, clip=None, steps=STEPS, check=False):
    """`steps` optimisation steps on one fixed batch from the same weights -> (p, m, v, costs, ema, facts).  facts['mults']:
    the multiplier read back from the device record after every step() call (not after capture_step's warm-up step)."""
    import bench
    dev = torch.device("cuda", 0)
    clips, targets, scores = bench.synth_batch(BATCH, 1000, dev)
    tr = bench.build_trainer(dev, seed=5)
    tr.lr = 1e-4
    tr.lr_schedule, tr.ema_decay, tr.clip_grad_norm = schedule, ema, clip
    captures, inner = [], tr.capture_step

    def counted(*a, **kw):
        captures.append(kw)
        return inner(*a, **kw)
    tr.capture_step = counted
    prev = None if ema is None else tr._ema_buffer().clone()
    costs, mults, rates = [], [], []

    def after(t, record=True):
        nonlocal prev
        if check and record and tr._sched_on():
            mults.append(_record_matches(tr, t, f"{mode} step {t}"))
        rates.append(tr.lr)
        if ema is not None:
            if check:
                _ema_matches(tr, prev, t, mode)
            prev = tr.arena.ema.clone()
    done = 0
    if mode != "eager":
        tr.capture_step(clips, targets, scores, warmup=1, lanes=mode == "lanes")        # the warm-up step is a real step
        done = 1
        after(1, record=False)              # (the record already holds the values of the step the capture was made for)
    for k in range(done, steps):
        costs.append(float(tr.step(clips, targets, scores)[0]))
        after(k + 1)
    torch.cuda.synchronize()
    assert tr.step_count == steps
    facts = dict(kind=None if tr._graph is None else (tr._graph[0] if isinstance(tr._graph[0], str) else "graph"),
                 replayed=tr.replayed_steps, captures=len(captures), mults=mults, rates=rates, record=None if tr._bias_corr is None else tr._bias_corr.numel(),
                 has_ema=getattr(tr.arena, "ema", None) is not None, trainer=tr if ema is not None and mode == "eager" else None)
    a = tr.arena
    return a.flat.detach().clone(), a.m.detach().clone(), a.v.detach().clone(), costs, None if ema is None else a.ema.detach().clone(), facts


def _plain():
    if "plain" not in _RUNS:
        _RUNS["plain"] = _run("eager")
        f = _RUNS["plain"][5]
        assert f["record"] is None and not f["has_ema"] and f["rates"] == [1e-4] * 3      # no flag: no record, no array
    return _RUNS["plain"]


def _same_run(a, b, label):
    for x, y, name in zip(a[:3], b[:3], ("p", "m", "v")):
        assert torch.equal(x, y), f"{label}: {name} differs by {float((x - y).abs().max())}"
    assert a[3][-len(b[3]):] == b[3], (label, a[3], b[3])


@pytest.mark.parametrize("mode", ["eager", "graph", "lanes"])
def test_a_multiplier_of_one_changes_nothing(bf16, mode):
    run = _run(mode, schedule=dict(CONSTANT), check=True)
    _same_run(_plain(), run, f"constant schedule, {mode}")
    f = run[5]
    assert f["record"] == 4 and not f["has_ema"] and f["mults"] == [1.0] * (3 if mode == "eager" else 2)
    assert f["kind"] == (None if mode == "eager" else mode)


@pytest.mark.parametrize("warmup,distinct_replays", [(2, 2), (1, 3)])
def test_a_schedule_replays_one_capture(bf16, warmup, distinct_replays):
    """Cosine, T = 6, lane graphs, four steps: capture_step is entered once, the three steps behind it replay that capture, and
    each ran at the multiplier of its own step, read back from the device record.

    W = 2 is the case as it was set.  By the rule its multipliers at t = 1..4 are 1/2, 1, 1, 3/4 (tau = 0 at t = W + 1): the four
    steps see three different rates, the three replays two.  W = 1 (1, 1 -> tau 0, 0.854, 0.5 at t = 2, 3, 4) is added so that
    three CONSECUTIVE replays at three different rates are checked as well."""
    sch = dict(COSINE, warmup_steps=warmup)
    run = _run("lanes", schedule=sch, steps=4, check=True)
    f = run[5]
    assert f["captures"] == 1 and f["replayed"] == 3 and f["kind"] == "lanes"
    want = [float(F32(S.multiplier(t=t, **sch))) for t in (1, 2, 3, 4)]
    assert f["mults"] == want[1:]                       # the three replays, each at the multiplier of its own step
    assert len(set(want)) == 3 and len(set(want[1:])) == distinct_replays
    assert f["rates"] == [1e-4 * float(S.multiplier(t=t, **sch)) for t in (1, 2, 3, 4)]         # trainer.lr: a host float


@pytest.mark.parametrize("mode", ["graph", "lanes"])
def test_scheduled_trajectory_is_the_same_in_every_launch_mode(bf16, mode):
    if "cosine_eager" not in _RUNS:
        _RUNS["cosine_eager"] = _run("eager", schedule=dict(COSINE), check=True)
        assert _RUNS["cosine_eager"][5]["mults"] == [0.5, 1.0, 1.0]
        assert not torch.equal(_RUNS["cosine_eager"][0], _plain()[0])                           # not the constant-rate run
    run = _run(mode, schedule=dict(COSINE), check=True)
    _same_run(_RUNS["cosine_eager"], run, f"cosine, {mode}")
    assert run[5]["kind"] == mode and run[5]["captures"] == 1


SPLIT_CODE = textwrap.dedent('''
    import os, sys, torch
    import torch.distributed as dist
    sys.path.insert(0, os.getcwd())
    import bench
    from opental_amd.common import ops
    ops.CONV_PRECISION = 1
    dev = torch.device("cuda", 0)
    dist.init_process_group(backend="nccl", device_id=dev)
    clips, targets, scores = bench.synth_batch(1, 1000, dev)
    def run(mode, steps=3):
        tr = bench.build_trainer(dev, seed=5, force_collectives=True)
        tr.lr = 1e-4
        tr.net.backbone._model.split_backward = True
        tr.lr_schedule, tr.ema_decay = dict(name="cosine", total_steps=6, warmup_steps=2), 0.9
        done = 0
        if mode == "split":
            tr.capture_step(clips, targets, scores, warmup=1, split=True)
            assert tr._graph[0] == "split"
            done = 1
        for _ in range(steps - done):
            tr.step(clips, targets, scores)
        torch.cuda.synchronize()
        assert tr.step_count == steps and tr._bias_corr.numel() == 4
        a = tr.arena
        return [t.detach().clone() for t in (a.flat, a.m, a.v, a.ema)], tr._bias_corr.cpu().tolist()
    eager, rec_e = run("eager")
    split, rec_s = run("split")
    assert rec_e == rec_s and rec_e[2] == 1.0, (rec_e, rec_s)
    for x, y, name in zip(eager, split, ("p", "m", "v", "ema")):
        assert torch.equal(x, y), (name, float((x - y).abs().max()))
    assert not torch.equal(eager[3], eager[0])
    print("OK", rec_s)
    dist.destroy_process_group()
''')


def test_scheduled_two_graph_step_equals_eager_steps_on_one_rccl_rank():
    """capture_step(split=True) with a schedule and the EMA: Adam runs eagerly behind the second graph and reads the record the
    host wrote before the first.  (Child process, one forced RCCL rank: a process group is global state.  The record is a
    host-computed value written identically on every rank, and no collective touches it.)"""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29617", RANK="0", WORLD_SIZE="1",
               HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    r = subprocess.run([sys.executable, "-c", SPLIT_CODE], cwd=REPO, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "OK" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


def test_ssl_step_beside_the_lane_graphs_runs_at_its_own_multiplier_and_the_next_step_replays(bf16):
    import bench
    from opental_amd.common import ops
    dev = torch.device("cuda", 0)
    clips, targets, scores = bench.synth_batch(BATCH, 1000, dev)
    ssl_clips, _, _ = bench.synth_batch(BATCH, 2000, dev)
    ssl_targets = [torch.tensor([[0.30, 0.55], [0.32, 0.52], [0.70, 0.90]], device=dev) * 256 for _ in range(BATCH)]
    sch = dict(name='cosine', total_steps=6, warmup_steps=1)            # multipliers 1, 1, 0.854, 0.5 at t = 1..4
    tr = bench.build_trainer(dev, seed=5)
    tr.lr = 1e-4
    tr.lr_schedule = sch
    tr.capture_step(clips, targets, scores, warmup=1, lanes=True)
    tr.step(clips, targets, scores)
    assert tr.replayed_steps == 1
    _record_matches(tr, 2, "replayed step")
    a = tr.arena
    p, m, v = a.flat.detach().clone(), a.m.detach().clone(), a.v.detach().clone()
    tr.step(clips, targets, scores, ssl_clips, ssl_targets)             # eager, beside the captured graphs
    assert tr.replayed_steps == 1 and tr.step_count == 3
    s3 = _record_matches(tr, 3, "ssl step")
    assert 0.85 < s3 < 0.86
    # ... and it IS Adam at the float32 product of rate and multiplier, on the gradient the step left
    bc = torch.tensor(ops.adam_bias_corrections(3, *tr.betas), dtype=torch.float32, device=dev)
    for lo, hi, g_lr in tr._group_ranges:
        g_lr = g_lr * (tr._lr / tr._base_lr)
        ops.adam_flat_dev(p[lo:hi], a.grad[lo:hi], m[lo:hi], v[lo:hi], bc, float(S.effective_lr32(g_lr, s3)), tr.betas[0], tr.betas[1],
                          tr.eps, tr.wd, grad_scale=1.0)
    torch.cuda.synchronize()
    assert not tr._skipped and torch.equal(p, a.flat) and torch.equal(m, a.m) and torch.equal(v, a.v)
    tr.step(clips, targets, scores)
    assert tr.replayed_steps == 2 and tr.step_count == 4 and tr._graph[0] == "lanes"
    assert _record_matches(tr, 4, "replayed step after the ssl step") == 0.5


@pytest.mark.parametrize("mode,clip", [("eager", None), ("lanes", None), ("lanes", 1e30)])
def test_ema_follows_the_weights_and_leaves_them_alone(bf16, mode, clip, tmp_path):
    run = _run(mode, ema=0.9, clip=clip, check=True)
    _same_run(_plain(), run, f"ema, {mode}, clip {clip}")               # (a clip value never reached leaves the run as it was)
    f = run[5]
    assert f["record"] == 4 and f["has_ema"] and set(f["mults"]) == {1.0} and f["rates"] == [1e-4] * 3
    if mode == "lanes":
        assert f["kind"] == "lanes" and f["replayed"] == 2 and f["captures"] == 1
        return
    # the averaged model as a state dict and as a file
    tr = f["trainer"]
    own, sd = tr.net.state_dict(), tr.ema_state_dict()
    assert len(sd) == 446 and list(sd) == list(own)
    offset = {id(p): off for p, off in zip(tr.arena.params, tr.arena.offsets)}
    names = {n: offset[id(p)] for n, p in tr.net.named_parameters() if id(p) in offset}
    assert sum(sd[n].numel() for n in names) == tr.arena.numel
    for k in sd:
        assert sd[k].shape == own[k].shape and sd[k].data_ptr() != own[k].data_ptr()
        if k in names:                      # an arena parameter: its EMA slice
            assert torch.equal(sd[k].reshape(-1), run[4][names[k]:names[k] + sd[k].numel()]), k
        else:                               # frozen BatchNorm tensors and buffers: as they are
            assert torch.equal(sd[k], own[k]), k
    assert sum(not torch.equal(sd[n], own[n]) for n in names) > len(names) // 2
    ckpt, state = str(tmp_path / "run"), str(tmp_path / "run" / "training")
    tr.save_model(3, ckpt, state)
    assert sorted(f_ for f_ in os.listdir(ckpt) if f_.endswith(".ckpt")) == ["checkpoint-3.ckpt", "checkpoint-ema-3.ckpt", "checkpoint-latest.ckpt"]
    assert list(torch.load(os.path.join(ckpt, "checkpoint-ema-3.ckpt"))) == list(torch.load(os.path.join(ckpt, "checkpoint-3.ckpt")))
    import bench
    new = bench.build_trainer(torch.device("cuda", 0), seed=9)
    new.ema_decay = 0.9
    new.resume_training(3, ckpt, state, restore_rng=False)
    assert new.ema_restored is True and new.step_count == 3
    assert torch.equal(new.arena.ema, run[4]) and torch.equal(new.arena.flat, run[0]) and torch.equal(new.arena.m, run[1])


# ------------------------------------------------------------------------------------------------ the drivers
OLD_KEYS = {'step', 'Train/Total', 'Train/loc', 'Train/conf', 'Train/prop_loc', 'Train/prop_conf', 'Train/IoU', 'Train/start',
            'Train/end'}


def _lines(ckpt):
    return [json.loads(l) for l in open(os.path.join(ckpt, "training", "scalars.jsonl")).read().splitlines()]


def _ckpts(directory):
    return sorted(f for f in os.listdir(directory) if f.endswith(".ckpt"))


def test_thumos_driver_schedules_logs_saves_and_scores_the_ema(tmp_path, bf16, capsys):
    from make_synthetic_thumos import CLASSES, make
    from opental_amd.thumos14 import score_checkpoints as SC, train as T
    data = str(tmp_path / "data")
    yaml_path = make(data, videos=1, frames=400, size=100)
    common = [yaml_path, '--open_set', '--split', '0', '--lw', '1', '--cw', '10', '--piou', '0.5', '--ssl', '0.001', '--batch_size', '2',
              '--random_init', '--max_steps', '3', '--max_epoch', '1', '--log_every', '1', '--save_after', '0']
    run_dir = str(tmp_path / "sched")
    tr, hist = T.main(common + ['--lr_schedule', 'cosine', '--min_lr_ratio', '0.1', '--ema_decay', '0.9', '--checkpoint_path', run_dir])
    base = tr._lr
    sch = dict(name='cosine', total_steps=tr.step_count, warmup_steps=0, min_lr_ratio=0.1, milestones=(), gamma=0.1)
    assert tr.lr_schedule == sch and tr.ema_decay == 0.9 and tr.step_count == T.steps_per_epoch(6, 2, 1, 3) == 3
    recs = _lines(run_dir)
    assert len(recs) == tr.step_count
    for r in recs:
        assert set(r) == OLD_KEYS | {'stats/lr'} and r['stats/lr'] == base * float(S.multiplier(t=r['step'], **sch))
    assert len({r['stats/lr'] for r in recs}) == 3 and recs[-1]['stats/lr'] == pytest.approx(0.1 * base, rel=1e-12)
    out = capsys.readouterr().out
    assert ", lr " in out and "lr schedule: cosine, 3 steps" in out and "weight EMA: decay 0.9" in out
    assert _ckpts(run_dir) == ['checkpoint-1.ckpt', 'checkpoint-ema-1.ckpt', 'checkpoint-latest.ckpt']
    saved = torch.load(os.path.join(run_dir, 'checkpoint-ema-1.ckpt'))
    assert len(saved) == 446 and list(saved) == list(torch.load(os.path.join(run_dir, 'checkpoint-1.ckpt')))
    # score_checkpoints --ema: a map file of its own, checkpoint_map.json neither read nor written
    # (a ground truth in which every class occurs, as the scoring asks: each tiles the first 30 s of both test videos)
    gt_file = os.path.join(data, 'gt_dense.json')
    database = {f"video_test_{v:07d}": dict(subset="test", duration=40.0, annotations=[
        dict(label=name, segment=[5.0 * k + 0.2 * c, 5.0 * (k + 1) + 0.2 * c]) for c, (_, name) in enumerate(CLASSES) for k in range(6)])
        for v in range(2)}
    json.dump(dict(database=database), open(gt_file, "w"))
    argv = [yaml_path, '--open_set', '--split', '0', '--checkpoint_path', run_dir, '--gt', gt_file,
            '--known', os.path.join(data, 'classes.txt')]
    map_file, result = SC.main(argv + ['--ema'])
    assert map_file == os.path.join(run_dir, 'checkpoint_map_ema.json') and os.path.exists(map_file)
    assert sorted(result) == ['1', 'best'] and len(result['1']['mAP']) == 5
    assert not os.path.exists(os.path.join(run_dir, 'checkpoint_map.json'))
    # without the flags: the records, the console and the files of before
    plain_dir = str(tmp_path / "plain")
    capsys.readouterr()
    tr, _ = T.main(common + ['--checkpoint_path', plain_dir])
    assert tr.lr_schedule is None and tr.ema_decay is None and (tr._bias_corr is None or tr._bias_corr.numel() == 2)
    assert getattr(tr.arena, 'ema', None) is None
    recs = _lines(plain_dir)
    assert len(recs) == tr.step_count and all(set(r) == OLD_KEYS for r in recs)
    out = capsys.readouterr().out
    assert " lr " not in out.replace("learning rate", "") and "EMA" not in out
    assert _ckpts(plain_dir) == ['checkpoint-1.ckpt', 'checkpoint-latest.ckpt']


def test_anet_driver_scales_both_groups_and_writes_the_ema_file(tmp_path, bf16):
    from make_synthetic_anet import make
    from opental_amd.anet import train as A
    yaml_path = make(str(tmp_path / "data"), videos=2, size=100)
    common = [yaml_path, '--open_set', '--split', '0', '--lw', '1', '--cw', '1', '--piou', '0.6', '--batch_size', '1',
              '--random_init', '--max_steps', '3', '--max_epoch', '1', '--log_every', '1', '--save_after', '0']
    run_dir = str(tmp_path / "sched")
    tr, _ = A.main(common + ['--lr_schedule', 'cosine', '--min_lr_ratio', '0.5', '--ema_decay', '0.99', '--checkpoint_path', run_dir])
    sch = tr.lr_schedule
    assert sch['name'] == 'cosine' and sch['total_steps'] == tr.step_count >= 1 and sch['min_lr_ratio'] == 0.5
    rates = sorted(g for _, _, g in tr._group_ranges)
    assert len(rates) == 2 and rates[0] == pytest.approx(rates[1] * 0.1)        # the backbone keeps lr / 10 as a launch argument
    recs = _lines(run_dir)
    assert len(recs) == tr.step_count
    assert all(set(r) == OLD_KEYS | {'stats/lr'} and r['stats/lr'] == tr._lr * float(S.multiplier(t=r['step'], **sch)) for r in recs)
    assert _ckpts(run_dir) == ['checkpoint-1.ckpt', 'checkpoint-ema-1.ckpt', 'checkpoint-latest.ckpt']
    st = torch.load(os.path.join(run_dir, 'training', 'checkpoint_1.ckpt'), weights_only=False)['optimizer']['param_groups']
    assert [g['initial_lr'] for g in st] == [g_lr for _, g_lr in tr.param_groups]
    assert all(g['lr'] == pytest.approx(g['initial_lr'] * float(tr.lr_multiplier(tr.step_count)), rel=1e-12) for g in st)
    plain_dir = str(tmp_path / "plain")
    tr, _ = A.main(common + ['--checkpoint_path', plain_dir])
    recs = _lines(plain_dir)
    assert len(recs) == tr.step_count and all(set(r) == OLD_KEYS for r in recs)
    assert _ckpts(plain_dir) == ['checkpoint-1.ckpt', 'checkpoint-latest.ckpt']
