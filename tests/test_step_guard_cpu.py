"""CPU: the non-finite-gradient guard's rule (opental_amd/common/step_guard.py) -- the bias-correction recurrence against
ops.adam_bias_corrections, the gate at the decision's edges, the guarded Adam trajectory against torch.optim.Adam stepped only
on the finite steps (what GradScaler does) --, the drivers' two flags, the step log's tenth value, the checkpoint round trip on
a CPU stand-in of the device record, and the two C prototypes."""
import ctypes
import importlib
import json
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import grad_norm_cases as GC
import step_guard_cases as SC
from opental_amd.common import step_guard as G

F32 = np.float32


# ------------------------------------------------------------------------------------------------ the rule
@pytest.mark.parametrize("betas", SC.BETAS)
def test_recurrence_gives_the_bits_of_the_pow_form_for_ten_thousand_steps(betas):
    from opental_amd.common import ops
    b1, b2 = np.float64(F32(betas[0])), np.float64(F32(betas[1]))
    p1, p2 = np.float64(1.0), np.float64(1.0)
    for t in range(1, 10001):
        p1, p2 = p1 * b1, p2 * b2
        got = G.corrections(p1, p2)
        want = ops.adam_bias_corrections(t, *betas)
        assert got[0].dtype == F32 and got[1].dtype == F32
        assert SC.same_bits(got[0], F32(want[0])) and SC.same_bits(got[1], F32(want[1])), (betas, t, got, want)
    # bias_powers IS that loop
    for t in (0, 1, 2, 77, 10000):
        q1, q2 = G.bias_powers(t, *betas)
        r1, r2 = np.float64(1.0), np.float64(1.0)
        for _ in range(t):
            r1, r2 = r1 * b1, r2 * b2
        assert q1 == r1 and q2 == r2 and isinstance(q1, np.float64)
    assert (p1, p2) == G.bias_powers(10000, *betas)
    with pytest.raises(ValueError):
        G.bias_powers(-1, *betas)


def test_record_layout_is_the_headers():
    from opental_amd import _lib
    text = open(_lib.HEADER_PATH).read()
    assert "#define OTAL_STEP_GUARD_BYTES 64" in text and "#define OTAL_STEP_GATE_MAX_STATE 4096" in text
    assert "#define OTAL_ABI_VERSION 26" in text
    assert G.BYTES == 64 and G.MAX_STATE == 4096 and G.RECORD.itemsize == 64
    assert [(n, G.RECORD.fields[n][1]) for n in ('applied', 'nonfinite', 'pow1', 'pow2', 'apply')] == \
        [('applied', 0), ('nonfinite', 8), ('pow1', 16), ('pow2', 24), ('apply', 32)]
    r = G.new_record()
    assert SC.record_bytes(r).tolist() == [0, 0, np.float64(1.0).view(np.int64), np.float64(1.0).view(np.int64), 0, 0, 0, 0]
    r = G.new_record(3, 2, 0.5, 0.9)
    assert (int(r['applied']), int(r['nonfinite']), float(r['pow1'])) == (3, 2, 0.125)
    b = np.float64(F32(0.9))
    assert r['pow2'] == (np.float64(1.0) * b) * b * b
    assert SC.record_from_bytes(SC.record_bytes(r)) == r
    assert "overflows float32" in G.__doc__


@pytest.mark.parametrize("betas", SC.BETAS)
def test_gate_applies_finite_norms_and_skips_the_rest(betas):
    b1, b2 = np.float64(F32(betas[0])), np.float64(F32(betas[1]))
    for norm in SC.FINITE_NORMS:
        start = G.new_record(5, 2, *betas)
        apply, r = G.gate(norm, start, *betas)
        assert apply is True
        assert (int(r['applied']), int(r['nonfinite']), int(r['apply'])) == (6, 2, 1)
        assert r['pow1'] == start['pow1'] * b1 and r['pow2'] == start['pow2'] * b2 and not r['reserved'].any()
        assert int(start['applied']) == 5                               # (nothing is modified in place)
    for norm in SC.BAD_NORMS:
        start = G.new_record(5, 2, *betas)
        apply, r = G.gate(norm, start, *betas)
        assert apply is False
        assert (int(r['applied']), int(r['nonfinite']), int(r['apply'])) == (5, 3, 0)
        assert r['pow1'] == start['pow1'] and r['pow2'] == start['pow2'] and not r['reserved'].any()
    # the long form: the step record and the loss state
    state, keep = SC.state_pair(50)
    host = np.asarray([9.0, 9.0, 0.25, 0.875], dtype=F32)
    apply, r, ss, s2, k2 = G.gate(F32(2.0), G.new_record(0, 0, *betas), *betas, host_state=host, loss_state=state, loss_state_keep=keep)
    assert apply and SC.same_bits(ss[:2], np.asarray(G.corrections(b1, b2))) and ss[2] == F32(0.25) and ss[3] == F32(0.875)
    assert SC.same_bits(s2, state) and SC.same_bits(k2, state)
    apply, r, ss, s2, k2 = G.gate(F32(np.nan), G.new_record(0, 0, *betas), *betas, loss_state=state, loss_state_keep=keep)
    assert not apply and ss.tolist() == [0.0, 0.0, 1.0, 0.0] and SC.same_bits(s2, keep) and SC.same_bits(k2, keep)
    with pytest.raises(ValueError):
        G.gate(F32(1.0), G.new_record(), loss_state=state)


@pytest.mark.parametrize("wd,grad_scale", [(0.0, 1.0), (1e-3, 0.5)])
def test_guarded_adam_is_torch_adam_stepped_on_the_finite_steps_only(wd, grad_scale):
    """torch.optim.Adam (float64 CPU tensors, optimizer.step() called on the finite steps only -- GradScaler's behaviour) beside
    guarded_adam_reference(grad_norm_cases.adam32), step by step.  After every step torch's p, exp_avg, exp_avg_sq are set to the
    float32 trajectory's, so that each comparison is ONE float32 update from common inputs, which is what the existing Adam
    bound is about (test_grad_norm_cpu.py: 2 x 2^-24 x e, e the oracle's running error); torch's own `step` counter is never
    touched and supplies its bias corrections -- it must therefore be the count of APPLIED steps.  (The oracle's e counts
    |update| three times over and half of the factor 2 is unused by the float32 roundings, which covers the one rounding of
    each float32 bias correction that torch's double corrections do not make.)"""
    from oracle import head_ref as H
    n = 301
    lr, b1, b2, eps = 1e-3, 0.9, 0.999, 1e-8
    steps = SC.eight_steps(n, where=7)
    rs = np.random.RandomState(11)
    p, m, v = rs.randn(n).astype(F32), np.zeros(n, dtype=F32), np.zeros(n, dtype=F32)
    f = lambda s: float(F32(s))
    pt = torch.tensor(p.astype(np.float64), requires_grad=True)
    opt = torch.optim.Adam([pt], lr=f(lr), betas=(f(b1), f(b2)), eps=f(eps), weight_decay=f(wd))
    rec = G.new_record(0, 0, b1, b2)
    kw = dict(lr=lr, eps=eps, weight_decay=wd, grad_scale=grad_scale)
    applied = 0
    for k, g in enumerate(steps, 1):
        finite = bool(np.isfinite(g).all())
        assert finite == (k not in SC.BAD_STEPS)
        p1, m1, v1, rec = G.guarded_adam_reference(GC.adam32, [g], p, m, v, b1, b2, record=rec, **kw)
        if not finite:                                      # torch: optimizer.step() is not called
            assert p1 is p and m1 is m and v1 is v and int(rec['apply']) == 0
            continue
        applied += 1
        pt.grad = torch.tensor(g.astype(np.float64) * f(grad_scale))
        opt.step()
        st = opt.state[pt]
        assert int(st['step']) == applied == int(rec['applied'])
        bc = G.corrections(rec['pow1'], rec['pow2'])
        (_, ep), (_, em), (_, ev) = H.adam(p, g, m, v, lr, b1, b2, eps, wd, applied, grad_scale, bias_corr=bc)
        for got, want, e, name in ((p1, pt.detach().numpy(), ep, "p"), (m1, st['exp_avg'].numpy(), em, "m"),
                                   (v1, st['exp_avg_sq'].numpy(), ev, "v")):
            assert got.dtype == F32
            assert np.all(np.abs(got.astype(np.float64) - want) <= 2.0 * 2.0 ** -24 * e), (k, name)
        p, m, v = p1, m1, v1
        with torch.no_grad():
            pt.copy_(torch.from_numpy(p.astype(np.float64)))
            st['exp_avg'].copy_(torch.from_numpy(m.astype(np.float64)))
            st['exp_avg_sq'].copy_(torch.from_numpy(v.astype(np.float64)))
    assert (int(rec['applied']), int(rec['nonfinite'])) == (4, 4) and int(opt.state[pt]['step']) == 4
    # the whole list at once, and the finite steps alone through an unguarded loop: the same bits
    p0 = rs.randn(n).astype(F32); z = np.zeros(n, dtype=F32)
    pa, ma, va, ra = G.guarded_adam_reference(GC.adam32, steps, p0, z, z, b1, b2, **kw)
    pb, mb, vb = p0, z, z
    from opental_amd.common import ops
    for t, g in enumerate(SC.finite_steps(steps), 1):
        pb, mb, vb = GC.adam32(pb, g, mb, vb, beta1=b1, beta2=b2, bias_corr=ops.adam_bias_corrections(t, b1, b2), **kw)
    assert SC.same_bits(pa, pb) and SC.same_bits(ma, mb) and SC.same_bits(va, vb) and int(ra['nonfinite']) == 4


def test_a_norm_that_overflows_float32_skips_a_finite_gradient():
    g = np.full(4, 2e38, dtype=F32)
    assert np.isfinite(g).all()
    p = np.ones(4, dtype=F32); z = np.zeros(4, dtype=F32)
    p1, _, _, r = G.guarded_adam_reference(GC.adam32, [g], p, z, z)
    assert p1 is p and (int(r['applied']), int(r['nonfinite'])) == (0, 1)


# ------------------------------------------------------------------------------------------------ flags
@pytest.mark.parametrize("module", ["thumos14", "anet"])
def test_drivers_refuse_a_limit_without_the_guard_and_a_limit_that_is_no_count(module):
    main = importlib.import_module(f"opental_amd.{module}.train").main
    with pytest.raises(SystemExit) as err:
        main(["some.yaml", "--max_nonfinite", "3"])
    assert "--max_nonfinite belongs to --skip_nonfinite" in str(err.value)
    for bad in (["-1"], ["2.5"], ["abc"], []):
        with pytest.raises(SystemExit) as err:
            main(["some.yaml", "--skip_nonfinite", "--max_nonfinite"] + bad)
        assert "--max_nonfinite takes a whole number >= 0" in str(err.value)
    assert "--skip_nonfinite" in main.__doc__ and "--max_nonfinite" in main.__doc__


def test_flags_parse_and_a_run_without_them_builds_its_trainer_as_before():
    from opental_amd.thumos14 import train as T
    extra = dict(G.GUARD_FLAGS)
    assert extra == {'skip_nonfinite': False, 'max_nonfinite': None}
    assert G.take_guard_flag(["x.yaml", "--lw", "1"], 1, extra) is None and extra == G.GUARD_FLAGS
    G.check_guard_flags(extra)
    assert T.guard_kwargs(extra) == {} and T.guard_log_kwargs(extra) == {}          # no keyword reaches DetectorTrainer / the log
    assert G.take_guard_flag(["--skip_nonfinite", "--lw"], 0, extra) == 0 and extra['skip_nonfinite'] is True
    assert G.take_guard_flag(["a", "--max_nonfinite", "0", "b"], 1, extra) == 2 and extra['max_nonfinite'] == 0
    G.check_guard_flags(extra)
    assert T.guard_kwargs(extra) == {'skip_nonfinite': True}
    assert T.guard_log_kwargs(extra) == {'with_guard': True, 'max_nonfinite': 0}
    assert T.guard_log_kwargs(extra, world=2) == {'with_guard': True, 'max_nonfinite': None}
    G.check_limit(0, 0); G.check_limit(5, None); G.check_limit(None, 3)
    with pytest.raises(SystemExit) as err:
        G.check_limit(1, 0)
    assert str(err.value) == G.limit_message(1, 0) and "--max_nonfinite 0" in str(err.value) and err.value.code != 0


def _tiny(**kw):
    from opental_amd.thumos14.train import DetectorTrainer
    torch.manual_seed(3)
    net = nn.Sequential(nn.Linear(3, 4), nn.Linear(4, 2))
    return DetectorTrainer(net, nn.Module(), dict(lw=1.0), lr=1e-3, weight_decay=0.0, **kw)


def test_trainer_argument_exists_defaults_to_off_and_joins_the_capture_key():
    import inspect
    from opental_amd.thumos14.train import DetectorTrainer
    assert inspect.signature(DetectorTrainer.__init__).parameters["skip_nonfinite"].default is False
    plain, on = _tiny(), _tiny(skip_nonfinite=True)
    assert plain.skip_nonfinite is False and not plain._norm_on() and len(plain._capture_key()) == 11
    assert on.skip_nonfinite is True and on._norm_on() and on._capture_key() != plain._capture_key()
    assert on._capture_key()[:11] == plain._capture_key()
    assert plain.guard_counts() == (0, 0)
    doc = DetectorTrainer.end_backward.__doc__
    assert "skip_nonfinite" in doc and "complete gradient" in doc


# ------------------------------------------------------------------------------------------------ the trainer's plumbing
class _RuleOps:
    """The three launches of a guarded step as the numpy rule on CPU tensors (the kernels themselves are held to the rule on
    the GPU): what the trainer hands them, in which order, is what this checks."""

    def __init__(self):
        self.calls = []

    def grad_norm(self, g, grad_scale, max_norm, out, partials):
        from opental_amd.common import grad_clip as R
        self.calls.append("norm")
        norm, coef = R.grad_norm_reference(g, grad_scale, max_norm)
        out.copy_(torch.tensor([float(norm), float(coef)]))
        return out

    def step_gate(self, norm, guard, step_state, beta1=0.9, beta2=0.999, host_state=None, loss_state=None, loss_state_keep=None):
        self.calls.append("gate")
        empty = np.zeros(0, dtype=F32)
        _, r, ss, s, k = G.gate(F32(norm[0].item()), SC.record_from_bytes(guard.numpy()), beta1, beta2,
                                host_state=None if host_state is None else host_state.numpy(),
                                loss_state=empty if loss_state is None else loss_state.numpy(),
                                loss_state_keep=empty if loss_state_keep is None else loss_state_keep.numpy())
        guard.copy_(torch.from_numpy(SC.record_bytes(r)))
        step_state.copy_(torch.from_numpy(ss))
        if loss_state is not None:
            loss_state.copy_(torch.from_numpy(s)); loss_state_keep.copy_(torch.from_numpy(k))

    def adam_flat_guard(self, p, g, m, v, step_state, guard, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, grad_scale=1.0,
                        ema=None, norm_coef=None):
        self.calls.append("adam")
        if int(SC.record_from_bytes(guard.numpy())['apply']) == 0:
            return
        ss = step_state.numpy()
        out = GC.adam32(p.numpy(), g.numpy(), m.numpy(), v.numpy(), lr=F32(lr) * ss[2], beta1=beta1, beta2=beta2, eps=eps,
                        weight_decay=weight_decay, bias_corr=(ss[0], ss[1]), grad_scale=grad_scale)
        with torch.no_grad():
            for t, new in zip((p, m, v), out):
                t.copy_(torch.from_numpy(new))
            if ema is not None:
                ema.copy_(ema + (p - ema) * float(F32(1.0) - ss[3]))


def _guarded_cpu_trainer(monkeypatch, **kw):
    from opental_amd.common import ops
    from opental_amd.thumos14.train import DetectorTrainer

    class Crit(nn.Module):
        """A criterion with a cross-step loss state that its forward pass advances, as the fused loss advances the IBM EMA."""
        cls_loss_type = 'edl'

        def __init__(self):
            super().__init__()
            self.cls_loss = nn.Module()
            self.cls_loss.register_buffer('weight_accum', torch.ones(5))
            self.cls_loss.state = lambda: self.cls_loss.weight_accum

    class CpuTrainer(DetectorTrainer):
        def compute_cost(self, clips, targets, scores, ssl_clips=None, ssl_targets=None):
            with torch.no_grad():
                self.criterion.cls_loss.weight_accum.mul_(0.5).add_(clips.abs().mean())
            cost = ((self.net(clips) - targets) ** 2).mean() * self.criterion.cls_loss.weight_accum.sum()
            return cost, (cost,)

    rule = _RuleOps()
    for name in ("grad_norm", "step_gate", "adam_flat_guard"):
        monkeypatch.setattr(ops, name, getattr(rule, name))
    torch.manual_seed(0)
    net = nn.Sequential(nn.Linear(8, 16), nn.ReLU(), nn.Linear(16, 1))
    return CpuTrainer(net, Crit(), {}, lr=1e-2, weight_decay=1e-3, distributed=False, skip_nonfinite=True, **kw), rule


@pytest.mark.parametrize("kw", [dict(), dict(ema_decay=0.1, lr_schedule=dict(name='constant', total_steps=10, warmup_steps=0))],
                         ids=["plain", "ema+schedule"])
def test_eager_steps_skip_a_poisoned_step_and_end_where_a_run_without_it_ends(monkeypatch, kw):
    g = torch.Generator().manual_seed(7)
    xs, ys = torch.randn(3, 5, 8, generator=g), torch.randn(3, 5, 1, generator=g)
    bad = ys[0].clone(); bad[2, 0] = float("nan")

    def snap(tr):
        a = tr.arena
        return [t.detach().clone() for t in (a.flat, a.m, a.v, tr._ibm_state())] + ([a.ema.clone()] if kw else [])
    tr, rule = _guarded_cpu_trainer(monkeypatch, **kw)
    tr.step(xs[0], ys[0], None)
    assert rule.calls == ["norm", "gate", "adam"]                       # the order within a step
    one = snap(tr)
    assert tr._state_keep is not None and torch.equal(tr._state_keep, tr._ibm_state())
    tr.step(xs[1], bad, None)                                           # a NaN target: a NaN cost, a NaN gradient
    assert not np.isfinite(float(tr.last_grad_norm[0]))
    assert all(torch.equal(a, b) for a, b in zip(one, snap(tr)))        # p, m, v, the loss state (and the EMA): the bits of before
    assert tr.guard_counts() == (1, 1) and tr.step_count == 2
    tr.step(xs[1], ys[1], None)
    tr.step(xs[2], ys[2], None)
    assert tr.guard_counts() == (3, 1) and tr.step_count == 4
    assert {float(s['step']) for s in tr.optimizer_state_dict()['state'].values()} == {3.0}
    clean, _ = _guarded_cpu_trainer(monkeypatch, **kw)
    for k in range(3):
        clean.step(xs[k], ys[k], None)
    assert clean.guard_counts() == (3, 0)
    assert all(torch.equal(a, b) for a, b in zip(snap(tr), snap(clean)))
    assert bool(torch.isfinite(tr.arena.flat).all())



OLD_KEYS = ['step', 'Train/Total', 'Train/loc', 'Train/conf', 'Train/prop_loc', 'Train/prop_conf', 'Train/IoU', 'Train/start',
            'Train/end']


def test_step_log_of_width_ten_carries_the_skipped_step_count(tmp_path, capsys):
    from opental_amd.thumos14.train import JsonlSink, StepLog, make_step_log
    log = make_step_log(1, str(tmp_path / "a"), with_guard=True)
    assert log.width == 10 and log.names == StepLog.NAMES + ('grad_norm', 'nonfinite')
    vec = torch.arange(10, dtype=torch.float32)
    vec[9] = 0.0
    log.push(1, vec)
    vec2 = vec.clone(); vec2[9] = 3.0
    log.push(2, vec2)
    log.poll(wait=True)
    log.sink.close()
    recs = [json.loads(l) for l in open(log.sink.path).read().splitlines()]
    assert [list(r) for r in recs] == [OLD_KEYS + ['stats/grad_norm', 'stats/nonfinite_steps']] * 2
    assert [r['stats/nonfinite_steps'] for r in recs] == [0, 3] and isinstance(recs[1]['stats/nonfinite_steps'], int)
    lines = capsys.readouterr().out.splitlines()
    assert lines[0].endswith("grad_norm 8.00000") and "nonfinite" not in lines[0]
    assert lines[1].endswith("grad_norm 8.00000, nonfinite 3")
    # the limit: the run ends where the record is flushed
    log = make_step_log(1, str(tmp_path / "b"), with_guard=True, max_nonfinite=2)
    log.push(1, vec)
    log.poll(wait=True)
    with pytest.raises(SystemExit) as err:
        log.push(2, vec2)
        log.poll(wait=True)
    assert str(err.value) == G.limit_message(3, 2)
    log.sink.close()
    assert len(open(log.sink.path).read().splitlines()) == 2            # the record that ended the run is in the file
    # without the guard the log is what it was
    assert make_step_log(1, str(tmp_path / "c"), with_norm=True).width == 9 and make_step_log(1, str(tmp_path / "d")).width == 8
    with pytest.raises(ValueError):
        StepLog(width=11)


# ------------------------------------------------------------------------------------------------ checkpoints
def test_checkpoint_round_trip_on_a_cpu_stand_in_of_the_record(tmp_path):
    tr = _tiny(skip_nonfinite=True)
    a = tr.arena
    torch.manual_seed(0)
    a.m.copy_(torch.randn_like(a.m)); a.v.copy_(torch.rand_like(a.v))
    tr.step_count = 9                                               # nine steps run: six applied, three skipped
    tr._guard = tr._guard_tensor(6, 3, 'cpu')
    rec = SC.record_from_bytes(tr._guard.numpy())
    assert rec == G.new_record(6, 3, *tr.betas) and tr.guard_counts() == (6, 3)
    sd = tr.optimizer_state_dict()
    assert {float(s['step']) for s in sd['state'].values()} == {6.0}            # what torch would hold
    ckpt, state = str(tmp_path / "c"), str(tmp_path / "c" / "training")
    tr.save_model(2, ckpt, state)
    st = torch.load(os.path.join(state, 'checkpoint_2.ckpt'), weights_only=False)
    assert st[G.CHECKPOINT_KEY] == {'applied': 6, 'nonfinite': 3}
    new = _tiny(skip_nonfinite=True)
    assert new.resume_training(2, ckpt, state, restore_rng=False) == 3
    assert new.step_count == 9 and new.guard_counts() == (6, 3) and new._guard is None
    assert torch.equal(new.arena.m, a.m) and torch.equal(new.arena.v, a.v)
    assert SC.record_from_bytes(new._guard_tensor(*new.guard_counts(), 'cpu').numpy()) == rec   # rebuilt by the recurrence
    # an unguarded trainer reads the file: Adam's step is the applied count
    plain = _tiny()
    plain.resume_training(2, ckpt, state, restore_rng=False)
    assert plain.step_count == 6 and plain.guard_counts() == (6, 0)
    # an old file (no key) is an unguarded run's: every step was applied
    old = _tiny()
    old.arena.m.copy_(a.m); old.arena.v.copy_(a.v)
    old.step_count = 5
    old.save_model(1, str(tmp_path / "o"), str(tmp_path / "o" / "training"))
    assert G.CHECKPOINT_KEY not in torch.load(os.path.join(str(tmp_path / "o"), "training", 'checkpoint_1.ckpt'), weights_only=False)
    new = _tiny(skip_nonfinite=True)
    new.resume_training(1, str(tmp_path / "o"), str(tmp_path / "o" / "training"), restore_rng=False)
    assert new.step_count == 5 and new.guard_counts() == (5, 0)
    assert G.counts_from_checkpoint({}, 5) == (5, 0) and G.counts_from_checkpoint({G.CHECKPOINT_KEY: {'applied': 2, 'nonfinite': 1}}, 2) == (2, 1)


# ------------------------------------------------------------------------------------------------ the C ABI
def test_header_declares_both_entries_with_the_specified_signatures():
    from opental_amd import _lib
    sigs = _lib.signatures()
    vp, f, i = ctypes.c_void_p, ctypes.c_float, ctypes.c_int
    # (norm, guard, host_state, step_state, beta1, beta2, loss_state, loss_state_keep, n_state, stream)
    assert sigs["otal_step_gate"] == (ctypes.c_int, [vp, vp, vp, vp, f, f, vp, vp, i, vp])
    sched = sigs["otal_adam_flat_sched"]
    assert sigs["otal_adam_flat_guard"] == (ctypes.c_int, sched[1][:-1] + [vp, vp])     # + guard in front of the stream


def test_library_exports_both_entries_and_refuses_bad_arguments_without_a_launch():
    from opental_amd import _lib
    from opental_amd.common import ops
    from opental_amd.csrc import build
    if not os.path.exists(build.LIB):
        build.build(verbose=False)
    lib = _lib.declare(ctypes.CDLL(build.LIB))
    one = ctypes.c_void_p(16)           # never dereferenced: the argument checks come first (there is no GPU here)
    NULL, SHAPE, UNSUPPORTED = -1, -2, -7
    assert lib.otal_step_gate(None, one, one, one, 0.9, 0.999, one, one, 4, None) == NULL
    assert lib.otal_step_gate(one, None, one, one, 0.9, 0.999, one, one, 4, None) == NULL
    assert lib.otal_step_gate(one, one, one, None, 0.9, 0.999, one, one, 4, None) == NULL
    assert lib.otal_step_gate(one, one, None, one, 0.9, 0.999, one, None, 4, None) == NULL     # a state without its keep buffer
    assert lib.otal_step_gate(one, one, one, one, 0.9, 0.999, one, one, -1, None) == SHAPE
    assert lib.otal_step_gate(one, one, one, one, 0.9, 0.999, one, one, G.MAX_STATE + 1, None) == UNSUPPORTED
    args = (4, 1e-3, 0.9, 0.999, 1e-8, 0.0)
    for k in range(4):
        ptrs = [one] * 4
        ptrs[k] = None
        assert lib.otal_adam_flat_guard(*ptrs, None, *args, one, 1.0, None, one, None) == NULL
    assert lib.otal_adam_flat_guard(one, one, one, one, None, *args, None, 1.0, None, one, None) == NULL
    assert lib.otal_adam_flat_guard(one, one, one, one, None, *args, one, 1.0, None, None, None) == NULL   # no guard
    assert lib.otal_adam_flat_guard(one, one, one, one, one, 0, *args[1:], one, 1.0, one, one, None) == SHAPE
    assert ops.STEP_GUARD_BYTES == G.BYTES and ops.STEP_GATE_MAX_STATE == G.MAX_STATE
    assert callable(ops.step_gate) and callable(ops.adam_flat_guard)
