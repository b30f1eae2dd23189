"""GPU: otal_step_gate / otal_adam_flat_guard against the rule of opental_amd/common/step_guard.py, bit for bit, and the
training step with `skip_nonfinite` in every launch mode (eager, one graph, lane graphs, two ranks, one forced RCCL rank with
the two-graph step) and through the two drivers.

Nothing here is approximate.  The gate's record, step record and loss-state copies are IEEE multiply / subtract / sqrt and
moves: the same bits as the numpy rule.  The guarded Adam shares otal_adam_flat_sched's body: torch.equal with it when the
step is applied, every byte (slack included) unchanged when it is skipped.  A trainer whose second step is poisoned must hold,
after it, the bits it held before it, and end where a run without that step ends.

The poison is a NaN written over the cached device vector of loss weights that the step's `torch.dot` reads at a fixed
address (thumos14.train._COST_WEIGHTS): the cost and with it every gradient element become NaN, in eager and replayed steps
alike.  A NaN is data; nothing here faults."""
import ctypes
import json
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

import step_guard_cases as SC
import test_head_kernels_gpu as HK
from opental_amd.common import step_guard as G

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
F32 = np.float32
NULL, SHAPE, UNSUPPORTED = -1, -2, -7


@pytest.fixture(scope="module")
def lib():
    from opental_amd import _lib as L
    return L.lib()


def _vp(t):
    return ctypes.c_void_p(t.data_ptr())


def _record_out(rec):
    """The 64-byte record in a guarded buffer (8 sentinel-framed 64-bit words, 16-byte aligned)."""
    o = HK.Out((8,), dtype=HK.F64, off=2)
    o.t.view(torch.int64).copy_(torch.from_numpy(SC.record_bytes(rec)))
    return o


def _record_of(o):
    return SC.record_from_bytes(o.t.view(torch.int64).cpu().numpy())


def _whole(o):
    return o.base.view(HK.INT[o.dtype]).clone()


# ------------------------------------------------------------------------------------------------ otal_step_gate
@pytest.mark.parametrize("with_host", [True, False], ids=["host_state", "no_host_state"])
@pytest.mark.parametrize("n_state", SC.STATE_SIZES)
def test_step_gate(lib, n_state, with_host):
    b1, b2 = 0.9, 0.999
    host0 = np.asarray([7.0, 7.0, 0.625, 0.96875], dtype=F32)
    for norm in SC.NORMS:
        start = G.new_record(5, 2, b1, b2)
        s0, k0 = SC.state_pair(max(n_state, 1))
        nrm = HK.Out((2,), init=np.asarray([norm, 0.5], dtype=F32))
        rec, host, step = _record_out(start), HK.Out((4,), init=host0), HK.Out((4,))
        state, keep = HK.Out((max(n_state, 1),), init=s0), HK.Out((max(n_state, 1),), off=5, init=k0)
        rc = lib.otal_step_gate(nrm.p(), rec.p(), host.p() if with_host else None, step.p(), b1, b2, state.p(), keep.p(),
                                n_state, HK.stream())
        assert rc == 0
        torch.cuda.synchronize()
        apply, want, ss, s1, k1 = G.gate(norm, start, b1, b2, host_state=host0 if with_host else None,
                                         loss_state=s0[:n_state], loss_state_keep=k0[:n_state])
        label = f"norm {norm!r} n_state {n_state}"
        for o, name in ((nrm, "norm"), (rec, "record"), (host, "host_state"), (step, "step_state"), (state, "state"), (keep, "keep")):
            o.check(f"{label}: {name}")                             # the words around every buffer keep their bits
        got = _record_of(rec)
        assert SC.record_bytes(got).tolist() == SC.record_bytes(want).tolist(), (label, got, want)
        assert int(got['apply']) == int(apply) == int(np.isfinite(norm))
        assert HK.same_bits(step.np(), ss), (label, step.np(), ss)
        assert HK.same_bits(nrm.np(), np.asarray([norm, 0.5], dtype=F32)) and HK.same_bits(host.np(), host0)
        assert HK.same_bits(state.np()[:n_state], s1) and HK.same_bits(keep.np()[:n_state], k1), label
        assert HK.same_bits(state.np()[n_state:], s0[n_state:]) and HK.same_bits(keep.np()[n_state:], k0[n_state:]), label


def test_step_gate_runs_the_recurrence_over_many_calls(lib):
    """Eight decisions in a row on one record: counts, powers and the step record after each are the rule's."""
    from opental_amd.common import ops
    b1, b2 = 0.95, 0.98
    rec = G.new_record(0, 0, b1, b2)
    dev_rec = torch.from_numpy(SC.record_bytes(rec)).cuda()
    step = torch.zeros(4, device="cuda")
    for k, norm in enumerate([np.inf, 1.0, 2.0, np.nan, -np.inf, 3.0, 0.0, np.nan], 1):
        ops.step_gate(torch.tensor([norm, 1.0], device="cuda"), dev_rec, step, b1, b2)
        _, rec, ss, _, _ = G.gate(F32(norm), rec, b1, b2, host_state=None, loss_state=np.zeros(0, dtype=F32),
                                  loss_state_keep=np.zeros(0, dtype=F32))
        assert dev_rec.cpu().numpy().tolist() == SC.record_bytes(rec).tolist(), k
        assert HK.same_bits(step.cpu().numpy(), ss), k
        if rec['apply']:
            want = ops.adam_bias_corrections(int(rec['applied']), b1, b2)
            assert HK.same_bits(ss[:2], np.asarray(want, dtype=F32))   # ... which are the host's pow() form's bits
    assert (int(rec['applied']), int(rec['nonfinite'])) == (4, 4)


def test_step_gate_refusals_write_nothing(lib):
    start = G.new_record(1, 1)
    nrm, rec, step = HK.Out((2,), init=np.asarray([1.0, 1.0], dtype=F32)), _record_out(start), HK.Out((4,))
    state, keep = HK.Out((8,)), HK.Out((8,))
    s = HK.stream()
    assert lib.otal_step_gate(None, rec.p(), None, step.p(), 0.9, 0.999, state.p(), keep.p(), 8, s) == NULL
    assert lib.otal_step_gate(nrm.p(), None, None, step.p(), 0.9, 0.999, state.p(), keep.p(), 8, s) == NULL
    assert lib.otal_step_gate(nrm.p(), rec.p(), None, None, 0.9, 0.999, state.p(), keep.p(), 8, s) == NULL
    assert lib.otal_step_gate(nrm.p(), rec.p(), None, step.p(), 0.9, 0.999, state.p(), None, 8, s) == NULL
    assert lib.otal_step_gate(nrm.p(), rec.p(), None, step.p(), 0.9, 0.999, state.p(), keep.p(), -1, s) == SHAPE
    assert lib.otal_step_gate(nrm.p(), rec.p(), None, step.p(), 0.9, 0.999, state.p(), keep.p(), G.MAX_STATE + 1, s) == UNSUPPORTED
    torch.cuda.synchronize()
    for o in (step, state, keep):
        o.check("refused gate", written=False)
    assert SC.record_bytes(_record_of(rec)).tolist() == SC.record_bytes(start).tolist()
    from opental_amd.common import ops
    with pytest.raises(RuntimeError):
        ops.step_gate(nrm.t, torch.zeros(4, dtype=torch.int64, device="cuda"), step.t)
    with pytest.raises(RuntimeError):
        ops.step_gate(nrm.t, torch.zeros(8, dtype=torch.int64, device="cuda"), step.t, loss_state=state.t)


# ------------------------------------------------------------------------------------------------ otal_adam_flat_guard
HYPER = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=1e-3)
STEP_STATE = np.asarray([1.0 - 0.9 ** 7, np.sqrt(1.0 - 0.999 ** 7), 0.75, 0.9], dtype=F32)


def _adam(lib, arrays, ema0, offs, coef, apply):
    """apply None: otal_adam_flat_sched; 1 / 0: otal_adam_flat_guard with that decision in its record.
    -> the five guarded buffers (ema None without one) and their whole contents before the call."""
    n = arrays[0].size
    h = HYPER
    bufs = [HK.Out((n,), off=o, init=a) for o, a in zip(offs, arrays)]
    ema = None if ema0 is None else HK.Out((n,), off=offs[0], init=ema0)
    ss = HK.dev(STEP_STATE)
    nc = None if coef is None else HK.dev(np.asarray([123.0, coef], dtype=F32))
    p, g, m, v = bufs
    before = [_whole(o) for o in bufs + ([ema] if ema is not None else [])]
    common = (p.p(), g.p(), m.p(), v.p(), None if ema is None else ema.p(), n, h["lr"], h["b1"], h["b2"], h["eps"], h["wd"], _vp(ss),
              0.5, None if nc is None else _vp(nc))
    if apply is None:
        rc = lib.otal_adam_flat_sched(*common, HK.stream())
    else:
        rec = G.new_record(6, 1)
        rec['apply'] = apply
        rec_dev = torch.from_numpy(SC.record_bytes(rec)).cuda()
        rc = lib.otal_adam_flat_guard(*common, _vp(rec_dev), HK.stream())
    assert rc == 0
    torch.cuda.synchronize()
    if apply is not None:
        assert rec_dev.cpu().numpy().tolist() == SC.record_bytes(rec).tolist()      # the record is read, never written
    return bufs + ([ema] if ema is not None else []), before


@pytest.mark.parametrize("offs", [(4, 4, 4, 4), (4, 5, 4, 4), (5, 4, 4, 4)], ids=["aligned", "g+1", "p+1"])
@pytest.mark.parametrize("n", (1, 3, 4, 5, 255, 256, 257, 1023, 1025))
def test_adam_flat_guard(lib, n, offs):
    import grad_norm_cases as GC
    arrays = GC.adam_state(n)
    ema0 = (arrays[0] * F32(0.75)).astype(F32)
    for with_ema in (False, True):
        for coef in (None, 0.37):
            e0 = ema0 if with_ema else None
            label = f"n {n} {offs} ema {with_ema} coef {coef}"
            want, _ = _adam(lib, arrays, e0, offs, coef, None)
            got, _ = _adam(lib, arrays, e0, offs, coef, 1)
            for a, b, name in zip(got, want, "pgmve"):
                a.check(f"{label}: {name}")
                assert torch.equal(a.t, b.t) and HK.same_bits(a.np(), b.np()), f"{label}: applied {name} differs from otal_adam_flat_sched"
            assert not HK.same_bits(got[0].np(), arrays[0])                  # (the update moved something)
            same, before = _adam(lib, arrays, e0, offs, coef, 0)
            for o, old, name in zip(same, before, "pgmve"):
                assert torch.equal(_whole(o), old), f"{label}: a skipped launch changed {name}"


def test_adam_flat_guard_refusals(lib):
    n = 8
    bufs = [HK.Out((n,)) for _ in range(5)]
    p, g, m, v, e = bufs
    ss, rec = HK.dev(STEP_STATE), torch.from_numpy(SC.record_bytes(G.new_record())).cuda()
    h = (1e-3, 0.9, 0.999, 1e-8, 0.0)
    s = HK.stream()
    assert lib.otal_adam_flat_guard(p.p(), g.p(), m.p(), v.p(), e.p(), n, *h, _vp(ss), 1.0, None, None, s) == NULL
    assert lib.otal_adam_flat_guard(p.p(), g.p(), m.p(), v.p(), e.p(), n, *h, None, 1.0, None, _vp(rec), s) == NULL
    assert lib.otal_adam_flat_guard(None, g.p(), m.p(), v.p(), e.p(), n, *h, _vp(ss), 1.0, None, _vp(rec), s) == NULL
    assert lib.otal_adam_flat_guard(p.p(), g.p(), m.p(), v.p(), e.p(), 0, *h, _vp(ss), 1.0, None, _vp(rec), s) == SHAPE
    torch.cuda.synchronize()
    for o in bufs:
        o.check("refused guard", written=False)


# ------------------------------------------------------------------------------------------------ a sequence through the C ABI
@pytest.mark.parametrize("where", [0, 1024, 1023], ids=["first", "last", "end_of_a_16_byte_group"])
def test_eight_steps_with_four_bad_ones_equal_the_four_finite_steps(lib, where):
    """grad_norm -> step_gate -> adam_flat_guard eight times (steps 1, 4, 5, 8 carry an inf or a NaN at `where`) against
    otal_adam_flat_sched on the four finite steps with the host's corrections for t = 1..4.  The lr multiplier and the keep
    factor follow the steps RUN (the host writes them per step), the corrections the steps APPLIED."""
    from opental_amd.common import ops
    n, b1, b2 = 1025, 0.9, 0.999
    steps = SC.eight_steps(n, where=where)
    rs = np.random.RandomState(5)
    p0 = rs.randn(n).astype(F32)
    mult = [F32(0.25 + 0.125 * k) for k in range(8)]
    keepf = [F32(0.5 + 0.0625 * k) for k in range(8)]
    kw = dict(lr=1e-3, beta1=b1, beta2=b2, eps=1e-8, weight_decay=1e-3, grad_scale=0.5)

    def fresh():
        return [HK.dev(p0), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda"), HK.dev((p0 * F32(0.5)).astype(F32))]
    p, m, v, ema = fresh()
    rec = torch.from_numpy(SC.record_bytes(G.new_record(0, 0, b1, b2))).cuda()
    norm, ws = torch.zeros(2, device="cuda"), torch.zeros(ops.GRAD_NORM_PARTIALS, dtype=torch.float64, device="cuda")
    step = torch.zeros(4, device="cuda")
    for k, g in enumerate(steps):
        gd = HK.dev(g)
        host = HK.dev(np.asarray([-1.0, -1.0, mult[k], keepf[k]], dtype=F32))       # (slots 0 and 1 are never read)
        ops.grad_norm(gd, 0.5, None, norm, ws)
        ops.step_gate(norm, rec, step, b1, b2, host_state=host)
        ops.adam_flat_guard(p, gd, m, v, step, rec, ema=ema, **kw)
    torch.cuda.synchronize()
    assert tuple(rec[:2].tolist()) == (4, 4)
    q, qm, qv, qema = fresh()
    t = 0
    for k, g in enumerate(steps):
        if not np.isfinite(g).all():
            continue
        t += 1
        bc = ops.adam_bias_corrections(t, b1, b2)
        ss = HK.dev(np.asarray([bc[0], bc[1], mult[k], keepf[k]], dtype=F32))
        ops.adam_flat_sched(q, HK.dev(g), qm, qv, ss, ema=qema, **kw)
    torch.cuda.synchronize()
    assert t == 4
    for a, b, name in ((p, q, "p"), (m, qm, "m"), (v, qv, "v"), (ema, qema, "ema")):
        assert torch.equal(a, b), f"bad element at {where}: {name} differs"
        assert bool(torch.isfinite(a).all())


# ------------------------------------------------------------------------------------------------ the trainer
BATCH = 1
EMA = 0.1           # below (1 + t) / (10 + t) at every t: one keep factor whatever the step's number, so that a run with a
_RUNS = {}          # skipped step and a run without that step move the EMA alike


@pytest.fixture()
def bf16():
    from opental_amd.common import ops
    old = ops.CONV_PRECISION
    ops.CONV_PRECISION = 1
    yield
    ops.CONV_PRECISION = old


class poisoned:
    """NaN over every cached loss-weight vector for the steps inside the block; the vectors get their values back."""

    def __enter__(self):
        from opental_amd.thumos14 import train as T
        torch.cuda.synchronize()
        self.saved = [(wv, wv.clone()) for wv in T._COST_WEIGHTS.values() if wv.is_cuda]
        assert self.saved, "no loss-weight vector is cached yet: run a step first"
        for wv, _ in self.saved:
            wv.fill_(float("nan"))
        return self

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        for wv, old in self.saved:
            wv.copy_(old)
        torch.cuda.synchronize()


def _snapshot(tr):
    a = tr.arena
    st = tr._ibm_state()
    return dict(p=a.flat.detach().clone(), m=a.m.detach().clone(), v=a.v.detach().clone(),
                ema=None if getattr(a, "ema", None) is None else a.ema.detach().clone(),
                state=None if st is None else st.detach().clone())


def _same(a, b, label, keys=("p", "m", "v", "ema", "state")):
    for k in keys:
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, (label, k)
            continue
        assert torch.equal(a[k], b[k]), f"{label}: {k} differs"


def _run(mode, guard, steps, poison_at=None, ema=None):
    """`steps` optimisation steps on one fixed batch from the same weights; step `poison_at` (1-based) runs with NaN loss
    weights.  -> dict(final snapshot, costs, after = {step: snapshot}, facts)."""
    import bench
    dev = torch.device("cuda", 0)
    clips, targets, scores = bench.synth_batch(BATCH, 1000, dev)
    tr = bench.build_trainer(dev, seed=5)
    tr.lr = 1e-4
    tr.skip_nonfinite, tr.ema_decay = guard, ema
    done = 0
    if mode != "eager":
        assert poison_at != 1
        tr.capture_step(clips, targets, scores, warmup=1, lanes=mode == "lanes")        # the warm-up step is a real step
        done = 1
    costs, after, bad_norm = [], {}, None
    for k in range(done + 1, steps + 1):
        if k == poison_at:
            after[k - 1] = _snapshot(tr)
            with poisoned():
                tr.step(clips, targets, scores)
                torch.cuda.synchronize()
                bad_norm = None if tr.last_grad_norm is None else float(tr.last_grad_norm[0])
            after[k] = _snapshot(tr)
        else:
            costs.append(float(tr.step(clips, targets, scores)[0]))
    torch.cuda.synchronize()
    facts = dict(kind=None if tr._graph is None else (tr._graph[0] if isinstance(tr._graph[0], str) else "graph"),
                 replayed=tr.replayed_steps, step_count=tr.step_count, counts=tr.guard_counts(), bad_norm=bad_norm,
                 adam_left=getattr(tr, "_adam_left", None), sd_step=None)
    if guard:
        facts["sd_step"] = {float(s["step"]) for s in tr.optimizer_state_dict()["state"].values()}
    return dict(final=_snapshot(tr), costs=costs, after=after, facts=facts)


def _plain():
    if "plain" not in _RUNS:
        _RUNS["plain"] = _run("eager", False, 3)
    return _RUNS["plain"]


def _clean_guarded(mode):
    if ("clean", mode) not in _RUNS:
        _RUNS[("clean", mode)] = _run(mode, True, 3, ema=EMA)
    return _RUNS[("clean", mode)]


@pytest.mark.parametrize("mode", ["eager", "graph", "lanes"])
def test_guard_without_a_bad_step_leaves_the_run_as_it_was(bf16, mode):
    plain, run = _plain(), _clean_guarded(mode)
    _same(plain["final"], run["final"], f"guarded, {mode}", keys=("p", "m", "v", "state"))
    assert plain["costs"][-len(run["costs"]):] == run["costs"], (plain["costs"], run["costs"])
    f = run["facts"]
    assert f["counts"] == (3, 0) and f["step_count"] == 3 and f["sd_step"] == {3.0}
    assert f["kind"] == (None if mode == "eager" else mode) and f["adam_left"] is None
    if mode == "lanes":
        assert f["replayed"] == 2
    assert plain["facts"]["counts"] == (3, 0)


@pytest.mark.parametrize("mode", ["eager", "graph", "lanes"])
def test_a_poisoned_second_step_is_skipped_and_leaves_no_trace(bf16, mode):
    run = _run(mode, True, 4, poison_at=2, ema=EMA)
    f = run["facts"]
    assert f["bad_norm"] is not None and not np.isfinite(f["bad_norm"]), f      # first: the poison reached the gradient
    _same(run["after"][1], run["after"][2], f"{mode}: across the skipped step")
    assert run["after"][1]["ema"] is not None
    print(f"{mode}: loss state carried: {run['after'][1]['state'] is not None}")
    _same(_clean_guarded(mode)["final"], run["final"], f"{mode}: four steps with one skipped vs three steps")
    assert run["costs"][-2:] == _clean_guarded(mode)["costs"][-2:]
    assert f["counts"] == (3, 1) and f["step_count"] == 4 and f["sd_step"] == {3.0}
    assert bool(torch.isfinite(run["final"]["p"]).all())
    if mode == "lanes":
        assert f["kind"] == "lanes" and f["replayed"] == 3                      # the bad step replayed too: nothing was re-captured
    if mode == "graph":
        assert f["kind"] == "graph"


def test_the_same_poison_ruins_an_unguarded_run(bf16):
    """The control: without the guard the poisoned step writes NaN into the parameters (this case does not depend on the
    feature; it shows that the poison is one)."""
    _plain()                                            # (a step has cached the loss weights)
    run = _run("eager", False, 2, poison_at=2)
    assert not bool(torch.isfinite(run["final"]["p"]).all()) and run["facts"]["counts"] == (2, 0)


RANK_CODE = textwrap.dedent('''
    import os, sys, torch
    import torch.distributed as dist
    sys.path.insert(0, os.getcwd())
    import bench
    from opental_amd.common import ops
    from opental_amd.thumos14 import train as T
    ops.CONV_PRECISION = 1
    rank, world, out = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"]), sys.argv[1]
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    dist.init_process_group(backend="gloo", rank=rank, world_size=world)
    tr = bench.build_trainer(dev, seed=5)
    assert tr.collectives and tr.world == world
    tr.lr = 1e-4
    tr.skip_nonfinite, tr.ema_decay = True, 0.1
    clips, targets, scores = bench.synth_batch(1, 1000 + rank, dev)
    tr.capture_step(clips, targets, scores, warmup=1, lanes=True)       # (the warm-up step is a real step)
    assert tr._graph[0] == "lanes"
    tr.step(clips, targets, scores)
    torch.cuda.synchronize()
    snap = lambda: [t.detach().clone() for t in (tr.arena.flat, tr.arena.m, tr.arena.v, tr.arena.ema)] + \\
        ([] if tr._ibm_state() is None else [tr._ibm_state().detach().clone()])
    before = snap()
    saved = [(w, w.clone()) for w in T._COST_WEIGHTS.values() if w.is_cuda]
    assert saved
    if rank == 1:                                       # ONE rank's loss is poisoned: the all-reduced gradient is NaN on both
        for w, _ in saved:
            w.fill_(float("nan"))
    tr.step(clips, targets, scores)
    torch.cuda.synchronize()
    for w, old in saved:
        w.copy_(old)
    bad = float(tr.last_grad_norm[0])
    unchanged = all(torch.equal(a, b) for a, b in zip(before, snap()))
    tr.step(clips, targets, scores)
    torch.cuda.synchronize()
    assert tr.step_count == 4 and tr.replayed_steps == 3
    torch.save({"flat": tr.arena.flat.cpu(), "m": tr.arena.m.cpu(), "ema": tr.arena.ema.cpu(), "counts": tr.guard_counts(),
                "bad": bad, "unchanged": unchanged, "moved": not torch.equal(before[0], tr.arena.flat)}, out + f".{rank}")
    dist.barrier()
    dist.destroy_process_group()
''')


def test_two_ranks_skip_together_when_one_ranks_gradient_is_not_finite(tmp_path):
    """Two rank processes on cuda:0 with gloo collectives (tests/test_dp_two_ranks_gpu.py's arrangement), the guard under
    lanes, rank 1 alone poisoned in step 3: both ranks read the same all-reduced bytes, both skip, the arenas stay equal."""
    out = str(tmp_path / "res")
    procs = []
    for r in range(2):
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29627", RANK=str(r), WORLD_SIZE="2")
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
    for r in res:
        assert not np.isfinite(r["bad"]) and r["unchanged"] and r["moved"] and tuple(r["counts"]) == (3, 1)
        assert bool(torch.isfinite(r["flat"]).all())
    for k in ("flat", "m", "ema"):
        assert torch.equal(res[0][k], res[1][k]), k


SPLIT_CODE = textwrap.dedent('''
    import os, sys, torch
    import torch.distributed as dist
    sys.path.insert(0, os.getcwd())
    import bench
    from opental_amd.common import ops
    from opental_amd.thumos14 import train as T
    ops.CONV_PRECISION = 1
    dev = torch.device("cuda", 0)
    dist.init_process_group(backend="nccl", device_id=dev)
    clips, targets, scores = bench.synth_batch(1, 1000, dev)
    def run(steps, poison_at):
        tr = bench.build_trainer(dev, seed=5, force_collectives=True)
        tr.lr = 1e-4
        tr.net.backbone._model.split_backward = True
        tr.skip_nonfinite = True
        tr.capture_step(clips, targets, scores, warmup=1, split=True)
        assert tr._graph[0] == "split"
        for k in range(2, steps + 1):
            if k != poison_at:
                tr.step(clips, targets, scores)
                continue
            torch.cuda.synchronize()
            before = [t.detach().clone() for t in (tr.arena.flat, tr.arena.m, tr.arena.v)]
            saved = [(w, w.clone()) for w in T._COST_WEIGHTS.values() if w.is_cuda]
            for w, _ in saved:
                w.fill_(float("nan"))
            tr.step(clips, targets, scores)
            torch.cuda.synchronize()
            for w, old in saved:
                w.copy_(old)
            assert not torch.isfinite(tr.last_grad_norm[0]), tr.last_grad_norm
            assert all(torch.equal(a, b) for a, b in zip(before, (tr.arena.flat, tr.arena.m, tr.arena.v)))
        torch.cuda.synchronize()
        assert tr._graph[0] == "split" and tr.step_count == steps
        return tr.arena.flat.detach().clone(), tr.arena.m.detach().clone(), tr.arena.v.detach().clone(), tr.guard_counts()
    pa, ma, va, ca = run(3, None)
    pb, mb, vb, cb = run(4, 3)
    assert ca == (3, 0) and cb == (3, 1), (ca, cb)
    assert torch.equal(pa, pb) and torch.equal(ma, mb) and torch.equal(va, vb), float((pa - pb).abs().max())
    assert bool(torch.isfinite(pb).all())
    print("OK", ca, cb)
    dist.destroy_process_group()
''')


def test_two_graph_step_on_one_rccl_rank_skips_a_poisoned_step():
    """capture_step(split=True) with the guard: the norm launch, the gate and the guarded Adam run eagerly behind the second
    graph and the stem's all-reduces.  (Child process, one forced RCCL rank: a process group is global state.)"""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29629", RANK="0", WORLD_SIZE="1",
               HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    r = subprocess.run([sys.executable, "-c", SPLIT_CODE], cwd=REPO, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "OK" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


# ------------------------------------------------------------------------------------------------ the drivers
OLD_KEYS = {'step', 'Train/Total', 'Train/loc', 'Train/conf', 'Train/prop_loc', 'Train/prop_conf', 'Train/IoU', 'Train/start',
            'Train/end'}
GUARD_KEYS = OLD_KEYS | {'stats/grad_norm', 'stats/nonfinite_steps'}


def _lines(ckpt):
    return [json.loads(l) for l in open(os.path.join(ckpt, "training", "scalars.jsonl")).read().splitlines()]


def _driver_case(main, common, tmp_path, capsys):
    tr, hist = main(common + ['--skip_nonfinite', '--checkpoint_path', str(tmp_path / "guard")])
    assert tr.skip_nonfinite and tr.last_grad_norm is not None and len(hist) == 1
    recs = _lines(str(tmp_path / "guard"))
    assert len(recs) == tr.step_count >= 1
    assert all(set(r) == GUARD_KEYS and r['stats/nonfinite_steps'] == 0 and r['stats/grad_norm'] > 0 for r in recs)
    assert tr.guard_counts() == (tr.step_count, 0)
    assert "nonfinite" not in capsys.readouterr().out                           # (the line names the count once it is > 0)
    tr, _ = main(common + ['--checkpoint_path', str(tmp_path / "plain")])
    assert not tr.skip_nonfinite and tr.last_grad_norm is None and tr._guard is None
    recs = _lines(str(tmp_path / "plain"))
    assert len(recs) == tr.step_count and all(set(r) == OLD_KEYS for r in recs)
    # every step poisoned, no skipped step allowed: the run ends at the first record it flushes
    with poisoned():
        with pytest.raises(SystemExit) as err:
            main(common + ['--skip_nonfinite', '--max_nonfinite', '0', '--checkpoint_path', str(tmp_path / "limit")])
    assert "more than --max_nonfinite 0 allows" in str(err.value) and "non-finite gradient" in str(err.value)
    assert err.value.code not in (0, None)
    recs = _lines(str(tmp_path / "limit"))
    assert recs and recs[-1]['stats/nonfinite_steps'] >= 1 and not np.isfinite(recs[-1]['stats/grad_norm'])
    assert "nonfinite " in capsys.readouterr().out


def test_thumos_driver_counts_skipped_steps_and_stops_at_the_limit(tmp_path, bf16, capsys):
    from make_synthetic_thumos import make
    from opental_amd.thumos14 import train as T
    yaml_path = make(str(tmp_path / "data"), videos=1, frames=400, size=100)
    common = [yaml_path, '--open_set', '--split', '0', '--lw', '1', '--cw', '10', '--piou', '0.5', '--ssl', '0.001', '--batch_size', '2',
              '--random_init', '--max_steps', '3', '--max_epoch', '1', '--log_every', '1']
    _driver_case(T.main, common, tmp_path, capsys)


def test_anet_driver_counts_skipped_steps_and_stops_at_the_limit(tmp_path, bf16, capsys):
    from make_synthetic_anet import make
    from opental_amd.anet import train as A
    yaml_path = make(str(tmp_path / "data"), videos=2, size=100)
    common = [yaml_path, '--open_set', '--split', '0', '--lw', '1', '--cw', '1', '--piou', '0.6', '--batch_size', '1',
              '--random_init', '--max_steps', '3', '--max_epoch', '1', '--log_every', '1']
    _driver_case(A.main, common, tmp_path, capsys)
