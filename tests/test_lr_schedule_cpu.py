"""CPU: the rule of opental_amd/common/lr_schedule.py against torch's own schedulers and torch.lerp, the header and the built
library's new entry, the drivers' flag parser, and the trainer's host side (capture key, checkpoints) on CPU tensors.
Tolerances: lr_schedule_cases.py."""
import ctypes
import json
import math
import os
import types
import warnings

import numpy as np
import pytest
import torch
import torch.nn as nn

import grad_norm_cases as GC
import lr_schedule_cases as LC
from opental_amd.common import grad_clip as R
from opental_amd.common import lr_schedule as S

F32 = np.float32
BASE_LR = 3e-4


def _torch_rates(make, steps):
    """The rate torch applies at optimisation steps 1..steps: the scheduler is stepped once per optimisation step."""
    opt = torch.optim.SGD([nn.Parameter(torch.zeros(1))], lr=BASE_LR)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sched = make(opt)
        out = []
        for _ in range(steps):
            out.append(opt.param_groups[0]['lr'])
            opt.step()
            sched.step()
    return out


def _warmup(opt, W):
    return torch.optim.lr_scheduler.LinearLR(opt, start_factor=1.0 / W, end_factor=1.0, total_iters=W - 1)


def _close(got, want):
    return abs(got - want) <= LC.REL * max(abs(want), 1e-300)


@pytest.mark.parametrize("T,W", LC.GRID)
def test_warmup_and_constant_are_torchs_linear_lr(T, W):
    if W >= 2:
        want = _torch_rates(lambda opt: _warmup(opt, W), T)
    else:                                   # W = 0 or 1: no step runs below the full rate (LinearLR(total_iters=0) divides by 0)
        want = [BASE_LR] * T
    for t in range(1, T + 1):
        got = BASE_LR * S.multiplier('constant', t, T, W)
        assert _close(got, want[t - 1]), (T, W, t, got, want[t - 1])
        if t <= W:
            assert S.multiplier('cosine', t, T, W) == S.multiplier('multistep', t, T, W, milestones=(1,)) == t / W


@pytest.mark.parametrize("r", [0.0, 0.1, 1.0])
@pytest.mark.parametrize("T,W", LC.GRID)
def test_cosine_is_torchs_cosine_annealing_behind_a_sequential_milestone(T, W, r):
    L = torch.optim.lr_scheduler
    tmax = max(1, T - W - 1)                # (T = W + 1: one step behind the warm-up, at tau = 0; torch divides by T_max)

    def make(opt):
        cos = L.CosineAnnealingLR(opt, T_max=tmax, eta_min=r * BASE_LR)
        if W < 2:                           # W = 1: the only warm-up step already runs at the full rate t / W = 1
            return L.SequentialLR(opt, [L.ConstantLR(opt, factor=1.0, total_iters=0), cos], milestones=[W]) if W else cos
        return L.SequentialLR(opt, [_warmup(opt, W), cos], milestones=[W])
    want = _torch_rates(make, T)
    for t in range(1, T + 1):
        got = BASE_LR * S.multiplier('cosine', t, T, W, min_lr_ratio=r)
        assert abs(got - want[t - 1]) <= LC.REL * BASE_LR, (T, W, r, t, got, want[t - 1])
    assert _close(S.multiplier('cosine', T, T, W, min_lr_ratio=r), r if T - W - 1 >= 1 else 1.0)


@pytest.mark.parametrize("T,W", LC.GRID)
def test_multistep_is_torchs_multistep_lr(T, W):
    milestones, gamma = (2, 5, 30), 0.3
    want = _torch_rates(lambda opt: torch.optim.lr_scheduler.MultiStepLR(opt, list(milestones), gamma=gamma), T)
    for t in range(W + 1, T + 1):           # (below the warm-up's end the warm-up rules: the test above)
        got = BASE_LR * S.multiplier('multistep', t, T, W, milestones=milestones, gamma=gamma)
        assert _close(got, want[t - 1]), (T, W, t, got, want[t - 1])
    assert S.multiplier('multistep', 3, 7, 0, milestones=(2,)) == 0.1 and S.multiplier('multistep', 2, 7, 0, milestones=(2,)) == 1.0


@pytest.mark.parametrize("T,W", LC.GRID)
def test_behind_the_last_step_the_last_value_holds(T, W):
    for name, kw in (('constant', {}), ('cosine', dict(min_lr_ratio=0.25)), ('multistep', dict(milestones=(1, 4), gamma=0.5))):
        last = S.multiplier(name, T, T, W, **kw)
        assert isinstance(last, np.float64)
        for t in (T + 1, T + 2, 10 * T):
            assert S.multiplier(name, t, T, W, **kw) == last


def test_bad_arguments_raise_value_error():
    for T, W in LC.REFUSED + [(5, 5), (5, 9)]:
        with pytest.raises(ValueError):
            S.multiplier('cosine', 1, T, W)
    for kw in (dict(name='linear'), dict(min_lr_ratio=-0.1), dict(min_lr_ratio=1.5), dict(milestones=(3, 3)), dict(milestones=(4, 2)),
               dict(t=0), dict(total_steps=0)):
        args = dict(dict(name='cosine', t=1, total_steps=10), **kw)
        with pytest.raises(ValueError):
            S.multiplier(**args)
    for decay in (-0.1, 1.0, 1.5, float('nan')):
        with pytest.raises(ValueError):
            S.ema_keep(decay, 1)


def test_what_the_device_sees():
    for t in (1, 2, 9, 90, 8999, 10 ** 6):
        k = S.ema_keep(0.999, t)
        assert isinstance(k, F32) and k == F32(min(0.999, (1 + t) / (10 + t)))
    # ((1 + t) / (10 + t) reaches 0.999 at t = 8990)
    assert S.ema_keep(0.999, 8000) < F32(0.999) and S.ema_keep(0.999, 8992) == F32(0.999) and S.ema_keep(0.0, 5) == 0
    lr = S.effective_lr32(1e-4, 0.37)
    assert isinstance(lr, F32) and GC.same_bits(lr, F32(1e-4) * F32(0.37)) and GC.same_bits(S.effective_lr32(1e-4, 1.0), F32(1e-4))
    rec = S.step_state((F32(0.1), F32(0.03)), 0.75, S.ema_keep(0.9, 3))
    assert rec.dtype == F32 and rec.tolist() == [float(F32(0.1)), float(F32(0.03)), 0.75, float(F32(4.0 / 13.0))]


# ------------------------------------------------------------------------------------------------ the update in float64
def _hyper():
    from oracle import head_ref as H
    return dict(beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-3, step=7, bias_corr=H.adam_bias_corrections(0.9, 0.999, 7))


@pytest.mark.parametrize("grad_scale,coef", [(1.0, None), (0.5, None), (0.5, F32(0.37)), (1.0, F32(1.0))])
def test_reference_at_multiplier_one_without_ema_is_the_clip_reference(grad_scale, coef):
    from oracle import head_ref as H
    p, g, m, v = GC.adam_state(3000, seed=2)
    got = S.adam_sched_reference(H.adam, p, g, m, v, grad_scale, 1e-3, 1.0, coef=coef, **_hyper())
    want = R.adam_clip_reference(H.adam, p, g, m, v, grad_scale, F32(1.0) if coef is None else coef, lr=1e-3, **_hyper())
    assert len(got) == 3
    for (a, ea), (b, eb) in zip(got, want):
        assert np.array_equal(a, b) and np.array_equal(ea, eb)
    # ... and a multiplier is the same statement at the float32 product of the two
    half = S.adam_sched_reference(H.adam, p, g, m, v, grad_scale, 1e-3, 0.37, coef=coef, **_hyper())
    want = R.adam_clip_reference(H.adam, p, g, m, v, grad_scale, F32(1.0) if coef is None else coef,
                                 lr=float(F32(1e-3) * F32(0.37)), **_hyper())
    assert np.array_equal(half[0][0], want[0][0]) and not np.array_equal(half[0][0], got[0][0])
    assert np.array_equal(half[1][0], got[1][0]) and np.array_equal(half[2][0], got[2][0])      # m, v do not see the rate


@pytest.mark.parametrize("keep", [0.0, 0.5, 0.999, float(S.ema_keep(0.999, 3))])
def test_reference_ema_line_is_torch_lerp_in_float64(keep):
    from oracle import head_ref as H
    p, g, m, v = GC.adam_state(3000, seed=3)
    ema = LC.ema_state(3000)
    out = S.adam_sched_reference(H.adam, p, g, m, v, 0.5, 1e-3, 0.8, ema=ema, keep=keep, **_hyper())
    assert len(out) == 4
    (pn, ep), (en, ee) = out[0], out[3]
    drop = float(F32(1.0) - F32(keep))
    want = torch.lerp(torch.from_numpy(ema.astype(np.float64)), torch.from_numpy(pn), drop).numpy()
    # (torch.lerp evaluates p - (p - ema) * (1 - w) for w >= 0.5: the same value up to float64 roundings)
    assert np.all(np.abs(en - want) <= 4 * 2.0 ** -53 * (np.abs(pn) + np.abs(ema)))
    assert np.all(ee >= ep * drop) and np.all(ee >= np.abs(en)) and np.all(np.isfinite(ee))
    # the float32 form of the line: within one ulp of the kernel's operation order restated in numpy
    p32 = pn.astype(F32)
    d = (p32 - ema).astype(F32)
    fma = (ema.astype(np.float64) + d.astype(np.float64) * drop).astype(F32)        # exact product, one rounding (+ the float64 sum's)
    assert LC.within_one_ulp(S.ema_reference(ema, p32, keep).astype(F32), fma)
    if keep == 0.0:
        assert np.array_equal(S.ema_reference(ema, p32, keep), ema.astype(np.float64) + d.astype(np.float64))


def test_ulp_distance():
    a = np.asarray([1.0, -1.0, 0.0, -0.0, np.nan, 1.0], dtype=F32)
    b = np.asarray([np.nextafter(F32(1.0), F32(2.0)), -1.0, -0.0, 0.0, np.nan, np.nan], dtype=F32)
    assert LC.ulp_distance(a, b).tolist()[:5] == [1, 0, 0, 0, 0] and LC.ulp_distance(a, b)[5] > 1
    assert LC.ulp_distance(np.asarray([2.0 ** -149], dtype=F32), np.asarray([-2.0 ** -149], dtype=F32))[0] == 2
    assert LC.sizes(GC.SIZES) == GC.SIZES[:-1] and LC.EXTRA_SIZE in LC.sizes(GC.SIZES)


# ------------------------------------------------------------------------------------------------ the C ABI
def test_header_declares_the_entry_and_the_library_exports_it():
    from opental_amd import _lib
    from opental_amd.common import ops
    from opental_amd.csrc import build
    vp, f, i64 = ctypes.c_void_p, ctypes.c_float, ctypes.c_int64
    sigs = _lib.signatures()
    # (p, g, m, v, ema, n, lr, beta1, beta2, eps, weight_decay, step_state, grad_scale, norm_coef, stream)
    assert sigs["otal_adam_flat_sched"] == (ctypes.c_int, [vp, vp, vp, vp, vp, i64, f, f, f, f, f, vp, f, vp, vp])
    assert "#define OTAL_ABI_VERSION 26" in open(_lib.HEADER_PATH).read()       # an additive entry
    if not os.path.exists(build.LIB):
        build.build(verbose=False)
    lib = _lib.declare(ctypes.CDLL(build.LIB))
    one = ctypes.c_void_p(16)               # never dereferenced: the argument checks come first (there is no GPU here)
    args = (4, 1e-3, 0.9, 0.999, 1e-8, 0.0)
    for k in range(4):
        ptrs = [None if j == k else one for j in range(4)]
        assert lib.otal_adam_flat_sched(*ptrs, one, *args, one, 1.0, one, None) == -1
    assert lib.otal_adam_flat_sched(one, one, one, one, None, *args, None, 1.0, None, None) == -1       # step_state
    assert lib.otal_adam_flat_sched(one, one, one, one, one, 0, *args[1:], one, 1.0, one, None) == -2
    assert lib.otal_adam_flat_sched(one, one, one, one, None, -3, *args[1:], one, 1.0, None, None) == -2
    assert callable(ops.adam_flat_sched)


# ------------------------------------------------------------------------------------------------ the drivers' flags
def _parse(argv):
    from opental_amd.thumos14 import train as T
    extra, rest, i = dict(T.LR_FLAGS), [], 0
    while i < len(argv):
        j = T.take_lr_flags(argv, i, extra)
        if j is None:
            rest.append(argv[i])
        else:
            i = j
        i += 1
    return extra, rest


def test_flag_parser_takes_its_words_and_leaves_the_rest():
    from opental_amd.thumos14 import train as T
    extra, rest = _parse(["x.yaml", "--lr_schedule", "multistep", "--lw", "1", "--lr_milestones", "3", "5", "--lr_gamma", "0.5",
                          "--warmup_steps", "4", "--ema_decay", "0.999", "y", "--min_lr_ratio", "0.1", "--open_set"])
    assert rest == ["x.yaml", "--lw", "1", "y", "--open_set"]
    assert extra == dict(lr_schedule='multistep', warmup_steps=4, min_lr_ratio=0.1, lr_milestones=[3, 5], lr_gamma=0.5, ema_decay=0.999)
    assert _parse(["x.yaml", "--lw", "1"]) == (dict(T.LR_FLAGS), ["x.yaml", "--lw", "1"])
    assert T.LR_FLAGS == dict(lr_schedule=None, warmup_steps=0, min_lr_ratio=0.0, lr_milestones=None, lr_gamma=0.1, ema_decay=None)
    for mod in ("thumos14", "anet"):
        import importlib
        doc = importlib.import_module(f"opental_amd.{mod}.train").main.__doc__
        assert all(flag in doc for flag in ("--lr_schedule", "--warmup_steps", "--min_lr_ratio", "--lr_milestones", "--lr_gamma", "--ema_decay"))


@pytest.mark.parametrize("module", ["thumos14", "anet"])
@pytest.mark.parametrize("flag,words,says", [
    ("--lr_schedule", ["linear"], "constant, cosine, multistep"), ("--lr_schedule", [], "constant, cosine, multistep"),
    ("--warmup_steps", ["-1"], "whole number"), ("--warmup_steps", ["2.5"], "whole number"), ("--warmup_steps", [], "whole number"),
    ("--min_lr_ratio", ["1.5"], "[0, 1]"), ("--min_lr_ratio", ["nan"], "[0, 1]"),
    ("--lr_milestones", [], "increasing epoch numbers"), ("--lr_milestones", ["3", "3"], "increasing epoch numbers"),
    ("--lr_milestones", ["0", "2"], "increasing epoch numbers"), ("--lr_milestones", ["a"], "increasing epoch numbers"),
    ("--lr_gamma", ["0"], "finite number > 0"), ("--lr_gamma", ["inf"], "finite number > 0"),
    ("--ema_decay", ["1"], "[0, 1)"), ("--ema_decay", ["-0.5"], "[0, 1)"), ("--ema_decay", ["x"], "[0, 1)"), ("--ema_decay", [], "[0, 1)")])
def test_drivers_end_with_a_sentence_for_a_bad_value(module, flag, words, says):
    import importlib
    main = importlib.import_module(f"opental_amd.{module}.train").main
    with pytest.raises(SystemExit) as err:
        main(["some.yaml", flag] + words + ["--lw", "1"])
    assert flag in str(err.value) and says in str(err.value), str(err.value)


def test_steps_per_epoch_and_the_schedule_of_a_command_line():
    from opental_amd.thumos14 import train as T
    assert T.steps_per_epoch(103, 4) == 25 and T.steps_per_epoch(103, 4, world=2) == 12 and T.steps_per_epoch(103, 4, world=8) == 3
    assert T.steps_per_epoch(103, 4, world=2, max_steps=5) == 5 and T.steps_per_epoch(103, 4, world=2, max_steps=50) == 12
    assert T.steps_per_epoch(3, 4) == 0
    # ... which is what run_one_epoch's batch list gives every rank (rank_batches, then the max_steps cut)
    for n, b, world, cap in ((103, 4, 2, None), (103, 4, 3, None), (26, 2, 4, 2), (7, 8, 1, None)):
        every = list(range(n // b))
        for rank in range(world):
            mine = T.rank_batches(every, rank, world)
            assert len(mine if cap is None else mine[:cap]) == T.steps_per_epoch(n, b, world, cap)
    extra, _ = _parse(["--lr_schedule", "multistep", "--lr_milestones", "2", "4", "--warmup_steps", "3"])
    assert T.lr_schedule_from_flags(extra, 5, 10) == dict(name='multistep', total_steps=50, warmup_steps=3, min_lr_ratio=0.0,
                                                          milestones=(20, 40), gamma=0.1)
    assert T.lr_schedule_from_flags(dict(T.LR_FLAGS), 5, 10) is None
    assert T.lr_schedule_from_flags(_parse(["--warmup_steps", "3"])[0], 5, 10)['name'] == 'constant'
    assert T.lr_schedule_from_flags(_parse(["--lr_schedule", "cosine", "--min_lr_ratio", "0.2"])[0], 2, 3) == dict(
        name='cosine', total_steps=6, warmup_steps=0, min_lr_ratio=0.2, milestones=(), gamma=0.1)
    for argv, says in ((["--lr_schedule", "multistep"], "--lr_milestones"), (["--lr_milestones", "2"], "multistep"),
                       (["--lr_schedule", "cosine", "--lr_milestones", "2"], "multistep"),
                       (["--lr_schedule", "cosine", "--warmup_steps", "50"], "warmup_steps")):
        with pytest.raises(SystemExit) as err:
            T.lr_schedule_from_flags(_parse(argv)[0], 5, 10)
        assert says in str(err.value)
    with pytest.raises(SystemExit) as err:
        T.lr_schedule_from_flags(_parse(["--lr_schedule", "cosine"])[0], 5, 0)
    assert "at least one" in str(err.value)


def test_jsonl_sink_writes_the_rate_only_when_asked(tmp_path, capsys):
    from opental_amd.thumos14.train import JsonlSink, make_step_log
    vec = torch.arange(8, dtype=torch.float32)
    log = make_step_log(1, str(tmp_path / "a"), lr_of=lambda step: 1e-4 * step)
    log.push(3, vec)
    log.poll(wait=True)
    log.sink.close()
    rec = json.loads(open(log.sink.path).read().splitlines()[0])
    assert list(rec)[-1] == 'stats/lr' == JsonlSink.LR_TAG and rec['stats/lr'] == 1e-4 * 3 and len(rec) == 10
    assert capsys.readouterr().out.rstrip().endswith("end 7.00000, lr 0.0003")
    log = make_step_log(1, str(tmp_path / "b"))
    log.push(3, vec)
    log.poll(wait=True)
    log.sink.close()
    assert 'stats/lr' not in json.loads(open(log.sink.path).read().splitlines()[0]) and " lr " not in capsys.readouterr().out


def test_score_checkpoints_lists_the_ema_files_apart(tmp_path):
    from opental_amd.common import score_checkpoints as SC
    for name in ("checkpoint-3.ckpt", "checkpoint-ema-3.ckpt", "checkpoint-ema-12.ckpt", "checkpoint-latest.ckpt", "checkpoint-ema-x.ckpt"):
        (tmp_path / name).write_bytes(b"")
    assert list(SC.list_checkpoints(str(tmp_path))) == [3]
    found = SC.list_checkpoints(str(tmp_path), ema=True)
    assert list(found) == [3, 12] and found[12].endswith("checkpoint-ema-12.ckpt")
    with pytest.raises(FileNotFoundError) as err:
        SC.list_checkpoints(str(tmp_path), [4], ema=True)
    assert "checkpoint-ema-" in str(err.value)
    assert SC.EMA_MAP_FILE == 'checkpoint_map_ema.json' and SC.FUSION_EMA_MAP_FILE == 'checkpoint_map_fusion_ema.json'
    assert "--ema" in SC.__doc__


# ------------------------------------------------------------------------------------------------ the trainer's host side
def _tiny(**kw):
    from opental_amd.thumos14.train import DetectorTrainer
    torch.manual_seed(3)
    net = nn.Sequential(nn.Linear(3, 4), nn.BatchNorm1d(4), nn.Linear(4, 2))
    net[1].weight.requires_grad_(False); net[1].bias.requires_grad_(False)      # frozen BatchNorm, as the backbone's
    return DetectorTrainer(net, nn.Module(), dict(lw=1.0), lr=1e-3, weight_decay=0.0, **kw)


COSINE = dict(name='cosine', total_steps=10, warmup_steps=2, min_lr_ratio=0.1)


def test_trainer_arguments_exist_and_default_to_off():
    import inspect
    from opental_amd.thumos14.train import DetectorTrainer
    sig = inspect.signature(DetectorTrainer.__init__).parameters
    assert sig["lr_schedule"].default is None and sig["ema_decay"].default is None
    tr = _tiny()
    assert tr.lr == 1e-3 and tr.lr_multiplier(5) == 1.0 and tr._step_record('cpu').numel() == 2 and tr._ema_buffer() is None
    assert len(tr._capture_key()) == 11 and tr._capture_key()[0] == 1e-3        # the key of a plain run is what it was
    assert all('initial_lr' not in g for g in tr.optimizer_state_dict()['param_groups'])
    with pytest.raises(RuntimeError):
        tr.ema_state_dict()
    for bad in (dict(lr_schedule=dict(name='linear', total_steps=5)), dict(lr_schedule=dict(name='cosine', total_steps=3, warmup_steps=3)),
                dict(lr_schedule=dict(name='cosine')), dict(ema_decay=1.0)):
        with pytest.raises(ValueError):
            _tiny(**bad)


def test_capture_key_holds_the_schedules_constants_not_the_current_rate():
    tr = _tiny(lr_schedule=dict(COSINE))
    keys, rates = [], []
    for t in (1, 2, 3, 6, 10):
        tr.step_count = t
        keys.append(tr._capture_key())
        rates.append(tr.lr)
    assert len(set(keys)) == 1 and len(set(rates)) == 4                         # (steps 2 and 3 both run at the full rate)
    assert rates == [1e-3 * float(S.multiplier(t=t, **COSINE)) for t in (1, 2, 3, 6, 10)]
    assert keys[0][0] == 1e-3 and keys[0][-1] == (('cosine', 10, 2, 0.1, (), 0.1), None)
    tr.lr = 2e-3                            # assigning sets the BASE rate: a new key
    assert tr._capture_key() != keys[0] and tr.lr == 2e-3 * float(S.multiplier(t=10, **COSINE))
    tr.lr = 1e-3
    assert tr._capture_key() == keys[0]
    other = [_tiny(lr_schedule=dict(COSINE, warmup_steps=3)), _tiny(lr_schedule=dict(COSINE), ema_decay=0.99), _tiny(ema_decay=0.99),
             _tiny(ema_decay=0.9), _tiny()]
    assert len({o._capture_key() for o in other} | {keys[0]}) == 6
    obj = _tiny(lr_schedule=types.SimpleNamespace(**COSINE))                    # a small object serves as the dict does
    assert obj._capture_key() == keys[0] and obj._step_record('cpu').numel() == 4


def test_optimizer_state_carries_initial_lr_and_the_ema_file_has_the_weights_keys(tmp_path):
    tr = _tiny(lr_schedule=dict(COSINE), ema_decay=0.9)
    a = tr.arena
    assert tr._ema_buffer() is a.ema and torch.equal(a.ema, a.flat) and a.ema.data_ptr() != a.flat.data_ptr()
    torch.manual_seed(0)
    a.ema.copy_(torch.randn_like(a.ema)); a.m.copy_(torch.randn_like(a.m)); a.v.copy_(torch.rand_like(a.v))
    tr.step_count = 6
    sd = tr.optimizer_state_dict()
    mult = float(S.multiplier(t=6, **COSINE))
    assert [g['initial_lr'] for g in sd['param_groups']] == [1e-3] and [g['lr'] for g in sd['param_groups']] == [1e-3 * mult] and mult < 1
    ema_sd = tr.ema_state_dict()
    assert list(ema_sd) == list(tr.net.state_dict()) and len(ema_sd) == 9
    for name, p in tr.net.named_parameters():
        if p.requires_grad:
            assert not torch.equal(ema_sd[name], p) and ema_sd[name].data_ptr() != p.data_ptr()
        else:
            assert torch.equal(ema_sd[name], p)
    assert torch.equal(ema_sd['1.running_var'], tr.net.state_dict()['1.running_var'])
    ckpt, state = str(tmp_path / "c"), str(tmp_path / "c" / "training")
    tr.save_model(4, ckpt, state)
    files = sorted(f for f in os.listdir(ckpt) if f.endswith('.ckpt'))
    assert files == ['checkpoint-4.ckpt', 'checkpoint-ema-4.ckpt', 'checkpoint-latest.ckpt']
    saved = torch.load(os.path.join(ckpt, 'checkpoint-ema-4.ckpt'))
    assert list(saved) == list(torch.load(os.path.join(ckpt, 'checkpoint-4.ckpt')))
    # a fresh trainer resumes: base rate from 'initial_lr', the schedule's position from Adam's step, the EMA bit for bit
    new = _tiny(lr_schedule=dict(COSINE), ema_decay=0.9)
    new.lr = 5.0
    assert new.resume_training(4, ckpt, state, restore_rng=False) == 5
    assert new._lr == 1e-3 and new._base_lr == 1e-3 and new.step_count == 6 and new.lr == 1e-3 * mult and new.ema_restored is True
    assert new._group_ranges == tr._group_ranges and new._capture_key() == tr._capture_key()
    assert torch.equal(new.arena.ema, a.ema) and torch.equal(new.arena.flat, a.flat) and torch.equal(new.arena.m, a.m)
    # without the EMA file the EMA starts from the resumed weights, and the trainer says so
    os.remove(os.path.join(ckpt, 'checkpoint-ema-4.ckpt'))
    new = _tiny(lr_schedule=dict(COSINE), ema_decay=0.9)
    new.resume_training(4, ckpt, state, restore_rng=False)
    assert new.ema_restored is False and torch.equal(new.arena.ema, new.arena.flat) and torch.equal(new.arena.flat, a.flat)
    said = []
    from opental_amd.thumos14.train import report_ema_resume
    report_ema_resume(new, 4, log=said.append)
    assert len(said) == 1 and "checkpoint-ema-4.ckpt" in said[0]
    # a run without the flags writes the files it wrote, and reads a scheduled run's state at its CURRENT rate's base
    plain = _tiny()
    plain.save_model(1, str(tmp_path / "p"), str(tmp_path / "p" / "training"))
    assert sorted(f for f in os.listdir(str(tmp_path / "p")) if f.endswith('.ckpt')) == ['checkpoint-1.ckpt', 'checkpoint-latest.ckpt']
    plain.resume_training(4, ckpt, state, restore_rng=False)
    assert plain.lr == 1e-3 and plain.ema_restored is None and getattr(plain.arena, 'ema', None) is None


def test_a_parameter_without_a_gradient_keeps_its_value_and_its_ema_moves_toward_it():
    tr = _tiny(ema_decay=0.9)
    a = tr.arena
    ema = tr._ema_buffer()
    torch.manual_seed(1)
    ema.copy_(torch.randn_like(ema))
    keep = S.ema_keep(0.9, 4)
    tr._bias_corr = torch.tensor(S.step_state((0.5, 0.5), 1.0, keep).tolist(), dtype=torch.float32)
    tr._skipped = [1]                       # the arena's second parameter received no gradient in this step
    sl = slice(a.offsets[1], a.offsets[1] + a.params[1].numel())
    before = [t.clone() for t in (a.flat, a.m, a.v, ema)]
    stash = tr._stash_skipped()
    assert len(stash) == 1 and len(stash[0]) == 5
    for t in (a.flat, a.m, a.v, ema):       # what the flat launch does to the whole arena, the skipped slice included
        t.add_(1.0)
    tr._restore_skipped(stash)
    for t, old in zip((a.flat, a.m, a.v), before):
        assert torch.equal(t[sl], old[sl])
        rest = torch.ones_like(t, dtype=torch.bool); rest[sl] = False
        assert torch.equal(t[rest], old[rest] + 1.0)
    # (torch ops, not the kernel's fmaf: the product and the sum round separately, half an ulp of each, beyond the rule's value)
    want = S.ema_reference(before[3][sl].numpy(), before[0][sl].numpy(), keep)
    moved = np.abs(want - before[3][sl].numpy().astype(np.float64))
    assert np.all(np.abs(ema[sl].numpy().astype(np.float64) - want) <= 2.0 ** -24 * (moved + np.abs(want)))
    assert not torch.equal(ema[sl], before[3][sl])
    # data parallel: where any peer used the parameter the update (and the launch's EMA) stays
    tr.collectives, tr._used_global = True, torch.tensor([1.0, 0.0, 2.0, 1.0])
    tr._skipped = [0, 1]
    before = [t.clone() for t in (a.flat, a.m, a.v, ema)]
    stash = tr._stash_skipped()
    for t in (a.flat, a.m, a.v, ema):
        t.add_(1.0)
    tr._restore_skipped(stash)
    s0 = slice(a.offsets[0], a.offsets[0] + a.params[0].numel())
    assert torch.equal(a.flat[s0], before[0][s0] + 1.0) and torch.equal(ema[s0], before[3][s0] + 1.0)      # used by a peer
    assert torch.equal(a.flat[sl], before[0][sl]) and not torch.equal(ema[sl], before[3][sl] + 1.0)       # used by nobody
    # without an EMA the stash is what it was
    plain = _tiny()
    plain._skipped = [0]
    assert len(plain._stash_skipped()[0]) == 4
