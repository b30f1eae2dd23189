"""CPU: the global-norm rule (opental_amd/common/grad_clip.py) against torch.nn.utils.clip_grad_norm_, the clipped Adam's
pre-scaled form against the flat Adam's arithmetic, the drivers' two flags, the capture key, the step log's ninth value and
the two C prototypes.  Reference: AFSD/thumos14/train.py:134-141,:248-250 (get_grad_norm -> 'stats/grad_norm', the clip line)."""
import ctypes
import json
import types

import numpy as np
import pytest
import torch

import grad_norm_cases as GC
from opental_amd.common import grad_clip as R

F32 = np.float32


def _torch_clip(g, max_norm):
    """-> (total_norm, coefficient) of torch.nn.utils.clip_grad_norm_ on one float32 CPU parameter whose gradient is g; the
    coefficient is read off an element that held exactly 1.0 (x * 1.0 is exact)."""
    assert g[0] == 1.0
    p = torch.nn.Parameter(torch.zeros(g.size))
    p.grad = torch.from_numpy(g.copy())
    total = torch.nn.utils.clip_grad_norm_([p], max_norm)
    assert total.dtype == torch.float32
    return F32(total.item()), F32(p.grad[0].item())


def _grad(kind="randn", n=1000, seed=3):
    g = GC.make_input(kind, n, seed)
    if kind in ("inf", "nan") and not np.isfinite(g[0]):
        g[1] = g[0]
    g[0] = 1.0
    return g


@pytest.mark.parametrize("n", [1, 5, 257, 1000])
def test_reference_norm_is_within_one_ulp_of_torch(n):
    """Sizes: clip_grad_norm_ adds the squares in float32, so ITS error grows with n (at n = 4097 it is two ulps from the
    correctly rounded norm); up to ~1000 terms it stays within one ulp of the exact value, and so must the float64 rule.
    Larger n: against torch's float64 norm, rounded once (next test)."""
    g = _grad(n=n)
    want, _ = _torch_clip(g, 1.0)
    got, _ = R.grad_norm_reference(g, 1.0, 1.0)
    assert got.dtype == F32 and GC.within_one_ulp(got, want), (got, want)
    half, _ = R.grad_norm_reference(g, 0.5, 0.0)
    assert GC.within_one_ulp(half, F32(want * F32(0.5)))            # (halving is exact)


@pytest.mark.parametrize("n", [4097, 100003])
def test_reference_norm_is_the_float64_norm_rounded_once(n):
    g = _grad(n=n)
    want = F32(torch.from_numpy(g).double().norm(2).item())
    got, _ = R.grad_norm_reference(g, 1.0, 0.0)
    assert GC.within_one_ulp(got, want), (got, want)


@pytest.mark.parametrize("seed", range(8))
def test_coefficient_equals_torch_bit_for_bit_below_at_and_above_one(seed):
    g = _grad(n=300 + seed, seed=seed)
    norm = float(_torch_clip(g, 1.0)[0])
    # below 1 (several, so that the two roundings of reciprocal() * max_norm show), at the edge, above (clamped to 1)
    for max_norm in [norm * f for f in (0.013, 0.1, 0.3, 0.37, 0.5, 0.77, 0.9, 0.999)] + \
                    [float(F32(norm) + F32(1e-6)), norm, norm * 1.0000001, norm * 2, 1e30]:
        total, coef = _torch_clip(g, max_norm)
        mine = R.clip_coefficient(total, max_norm)
        assert mine.dtype == F32 and GC.same_bits(mine, coef), (max_norm, total, mine, coef)
        assert mine <= 1.0
    assert R.clip_coefficient(F32(norm), norm * 2) == 1.0 and R.clip_coefficient(F32(norm), norm * 0.5) < 1.0


def test_norm_only_and_non_finite_gradients():
    g = _grad()
    for off in (0.0, -1.0, None):
        norm, coef = R.grad_norm_reference(g, 1.0, off)
        assert np.isfinite(norm) and GC.same_bits(coef, F32(1.0))
    # an inf entry: norm inf, coefficient 0 (torch: 1 / inf * max_norm)
    total, coef = _torch_clip(_grad("inf"), 5.0)
    norm, mine = R.grad_norm_reference(_grad("inf"), 1.0, 5.0)
    assert np.isinf(total) and np.isinf(norm) and norm > 0 and GC.same_bits(mine, coef) and mine == 0.0
    # a NaN entry: both NaN, as torch's clamp keeps it
    total, coef = _torch_clip(_grad("nan"), 5.0)
    norm, mine = R.grad_norm_reference(_grad("nan"), 1.0, 5.0)
    assert np.isnan(total) and np.isnan(coef) and np.isnan(norm) and np.isnan(mine)
    # zeros: norm 0, coefficient min(1, (1 / 1e-6) * max_norm)
    z = np.zeros(7, dtype=F32)
    assert R.grad_norm_reference(z, 1.0, 5.0) == (0.0, 1.0)
    norm, mine = R.grad_norm_reference(z, 1.0, 2.5e-7)
    assert norm == 0.0 and GC.same_bits(mine, F32(F32(1.0) / F32(1e-6)) * F32(2.5e-7)) and 0.2 < mine < 0.3
    # a square that overflows float32 but not float64
    norm, _ = R.grad_norm_reference(GC.make_input("big", 100), 1.0, 0.0)
    assert np.isfinite(norm) and GC.within_one_ulp(norm, F32(1e18))


def test_reference_takes_tensors_and_any_shape():
    g = _grad(n=600)
    a = R.grad_norm_reference(torch.from_numpy(g).view(20, 30), 0.5, 3.0)
    b = R.grad_norm_reference(g, 0.5, 3.0)
    assert GC.same_bits(a[0], b[0]) and GC.same_bits(a[1], b[1])


@pytest.mark.parametrize("grad_scale,wd", [(1.0, 0.0), (0.5, 1e-3), (0.25, 1e-3)])
def test_clipped_adam_with_coefficient_one_is_the_flat_adam(grad_scale, wd):
    from oracle import head_ref as H
    p, g, m, v = GC.adam_state(5000, seed=1)
    bc = H.adam_bias_corrections(0.9, 0.999, 7)
    kw = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=wd, bias_corr=bc)
    plain = GC.adam32(p, g, m, v, grad_scale=grad_scale, **kw)
    clipped = R.adam_clip_reference(GC.adam32, p, g, m, v, grad_scale, F32(1.0), **kw)
    for a, b in zip(plain, clipped):
        assert GC.same_bits(a, b)
    # ... and adam32 IS the existing oracle's arithmetic: within that oracle's own per-element bound of its float64 statement
    (rp, ep), (rm, em), (rv, ev) = H.adam(p, g, m, v, 1e-3, 0.9, 0.999, 1e-8, wd, 7, grad_scale)
    for got, ref, e in zip(plain, (rp, rm, rv), (ep, em, ev)):
        assert np.all(np.abs(got.astype(np.float64) - ref) <= 2.0 * 2.0 ** -24 * e)
    # a coefficient below one moves the result, and is what scaling the gradient first gives
    half = R.adam_clip_reference(GC.adam32, p, g, m, v, 1.0, F32(0.5), **kw)
    want = GC.adam32(p, (g * F32(0.5)).astype(F32), m, v, grad_scale=1.0, **kw)
    unclipped = GC.adam32(p, g, m, v, grad_scale=1.0, **kw)
    assert all(GC.same_bits(a, b) for a, b in zip(half, want)) and not GC.same_bits(half[0], unclipped[0])


# ------------------------------------------------------------------------------------------------ flags, capture key
@pytest.mark.parametrize("module", ["thumos14", "anet"])
@pytest.mark.parametrize("bad", ["0", "-1", "abc", "nan", "inf", None])
def test_drivers_refuse_a_clip_value_that_is_not_positive(module, bad):
    import importlib
    main = importlib.import_module(f"opental_amd.{module}.train").main
    with pytest.raises(SystemExit) as err:
        main(["some.yaml", "--clip_grad_norm"] + ([] if bad is None else [bad]))
    assert "--clip_grad_norm" in str(err.value)


def test_clip_flag_implies_logging():
    from opental_amd.thumos14.train import take_grad_norm_flag
    extra = {'clip_grad_norm': None, 'log_grad_norm': False}
    assert take_grad_norm_flag(["x.yaml", "--lw", "1"], 1, extra) is None and extra == {'clip_grad_norm': None, 'log_grad_norm': False}
    assert take_grad_norm_flag(["--log_grad_norm", "--lw"], 0, extra) == 0
    assert extra == {'clip_grad_norm': None, 'log_grad_norm': True}
    extra = {'clip_grad_norm': None, 'log_grad_norm': False}
    assert take_grad_norm_flag(["x.yaml", "--clip_grad_norm", "20", "--lw"], 1, extra) == 2
    assert extra == {'clip_grad_norm': 20.0, 'log_grad_norm': True}
    for mod in ("thumos14", "anet"):
        import importlib
        doc = importlib.import_module(f"opental_amd.{mod}.train").main.__doc__
        assert "--clip_grad_norm" in doc and "--log_grad_norm" in doc


def _key(clip=None, track=False, lr=1e-5):
    from opental_amd.thumos14.train import DetectorTrainer
    stub = types.SimpleNamespace(criterion=types.SimpleNamespace(cls_loss=None), lr=lr, _base_lr=1e-5, _group_ranges=[(0, 10, 1e-5)],
                                 wd=1e-3, betas=(0.9, 0.999), eps=1e-8, world=1, collectives=False, w=dict(lw=1.0, cw=10.0),
                                 clip_grad_norm=clip, track_grad_norm=track)
    return DetectorTrainer._capture_key(stub)


def test_capture_key_carries_the_clip_value_and_the_tracking_switch():
    assert _key() == _key() and _key(20.0, True) == _key(20.0, True)
    keys = [_key(), _key(track=True), _key(20.0), _key(20.0, True), _key(5.0), _key(5.0, True)]
    assert len(set(keys)) == len(keys)
    assert _key(lr=2e-5) != _key()


def test_trainer_arguments_exist_and_default_to_off():
    import inspect
    from opental_amd.thumos14.train import DetectorTrainer
    sig = inspect.signature(DetectorTrainer.__init__).parameters
    assert sig["clip_grad_norm"].default is None and sig["track_grad_norm"].default is False
    assert "global norm" in DetectorTrainer.end_backward.__doc__


# ------------------------------------------------------------------------------------------------ StepLog / JsonlSink
OLD_KEYS = ['step', 'Train/Total', 'Train/loc', 'Train/conf', 'Train/prop_loc', 'Train/prop_conf', 'Train/IoU', 'Train/start',
            'Train/end']


def test_step_log_defaults_are_the_eight_scalars(tmp_path):
    from opental_amd.thumos14.train import JsonlSink, StepLog
    assert StepLog.NAMES == ('total', 'loc', 'conf', 'prop_loc', 'prop_conf', 'IoU', 'start', 'end')
    assert JsonlSink.TAGS == ('Total', 'loc', 'conf', 'prop_loc', 'prop_conf', 'IoU', 'start', 'end')
    sink = JsonlSink(str(tmp_path))
    log = StepLog(every=1, sink=sink)
    assert log.width == 8 and log.names == StepLog.NAMES and all(buf.numel() == 8 for buf, _ in log._free)
    vec = torch.tensor([8.5, 1.0, 2.0, 3.0, 0.5, 0.25, 0.125, 1.625])
    log.push(3, vec)
    log.poll(wait=True)
    sink.close()
    assert log.records == [(3, vec.tolist())]
    want = {'step': 3}
    want.update({k: x for k, x in zip(OLD_KEYS[1:], vec.tolist())})
    lines = open(sink.path).read().splitlines()
    assert lines == [json.dumps(want)]                  # the line as it always was: same keys, same order, same text
    assert list(json.loads(lines[0])) == OLD_KEYS


def test_step_log_of_width_nine_carries_the_gradient_norm(tmp_path):
    from opental_amd.thumos14.train import JsonlSink, StepLog, make_step_log
    seen = []
    sink = JsonlSink(str(tmp_path), echo=lambda step, v: seen.append((step, list(v))))
    log = StepLog(every=1, sink=sink, width=9)
    assert log.names == StepLog.NAMES + ('grad_norm',) and all(buf.numel() == 9 for buf, _ in log._free)
    vec = torch.arange(9, dtype=torch.float32) + 0.5
    log.push(1, vec)
    log.poll(wait=True)
    sink.close()
    rec = json.loads(open(sink.path).read().splitlines()[0])
    assert list(rec) == OLD_KEYS + ['stats/grad_norm'] and rec['stats/grad_norm'] == 8.5 and rec['Train/end'] == 7.5
    assert seen == [(1, vec.tolist())]
    with pytest.raises(ValueError):
        StepLog(width=7)
    d = make_step_log(2, str(tmp_path / "d"), with_norm=True)
    assert d.width == 9 and d.every == 2 and isinstance(d.sink, JsonlSink)
    d.sink.close()
    assert make_step_log(2, str(tmp_path / "e")).width == 8


def test_console_line_names_the_gradient_norm(tmp_path, capsys):
    from opental_amd.thumos14.train import make_step_log
    log = make_step_log(1, str(tmp_path), with_norm=True)
    log.push(4, torch.arange(9, dtype=torch.float32))
    log.poll(wait=True)
    log.sink.close()
    out = capsys.readouterr().out
    assert out.startswith("step 4 total 0.00000, ") and out.rstrip().endswith("end 7.00000, grad_norm 8.00000")


# ------------------------------------------------------------------------------------------------ the C ABI
def test_header_declares_both_entries_with_the_specified_signatures():
    from opental_amd import _lib
    sigs = _lib.signatures()
    vp, f, i64 = ctypes.c_void_p, ctypes.c_float, ctypes.c_int64
    # (g, n, grad_scale, max_norm, partials, out, stream)
    assert sigs["otal_grad_norm"] == (ctypes.c_int, [vp, i64, f, f, vp, vp, vp])
    # otal_adam_flat_dev's parameters + norm_coef in front of the stream
    dev = sigs["otal_adam_flat_dev"]
    assert sigs["otal_adam_flat_clip"] == (ctypes.c_int, dev[1][:-1] + [vp, vp])
    assert dev == (ctypes.c_int, [vp, vp, vp, vp, i64, f, f, f, f, f, vp, f, vp])
    text = open(_lib.HEADER_PATH).read()
    assert "#define OTAL_GRAD_NORM_PARTIALS 2048" in text and "#define OTAL_ABI_VERSION 26" in text
    assert GC.GRID_CAP == 2048


def test_library_exports_both_entries_and_refuses_bad_arguments_without_a_launch():
    from opental_amd import _lib
    from opental_amd.common import ops
    from opental_amd.csrc import build
    import os
    if not os.path.exists(build.LIB):
        build.build(verbose=False)
    lib = _lib.declare(ctypes.CDLL(build.LIB))
    one = ctypes.c_void_p(16)           # never dereferenced: the argument checks come first (there is no GPU here)
    assert lib.otal_grad_norm(None, 4, 1.0, 0.0, one, one, None) == -1
    assert lib.otal_grad_norm(one, 4, 1.0, 0.0, None, one, None) == -1
    assert lib.otal_grad_norm(one, 4, 1.0, 0.0, one, None, None) == -1
    assert lib.otal_grad_norm(one, 0, 1.0, 0.0, one, one, None) == -2
    assert lib.otal_grad_norm(one, -5, 1.0, 0.0, one, one, None) == -2
    args = (4, 1e-3, 0.9, 0.999, 1e-8, 0.0)
    assert lib.otal_adam_flat_clip(one, one, one, one, *args, one, 1.0, None, None) == -1
    assert lib.otal_adam_flat_clip(one, one, one, one, *args, None, 1.0, one, None) == -1
    assert lib.otal_adam_flat_clip(None, one, one, one, *args, one, 1.0, one, None) == -1
    assert lib.otal_adam_flat_clip(one, one, one, one, 0, *args[1:], one, 1.0, one, None) == -2
    assert ops.GRAD_NORM_PARTIALS == GC.GRID_CAP and callable(ops.grad_norm) and callable(ops.adam_flat_clip)
