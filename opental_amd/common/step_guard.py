"""The non-finite-gradient guard of the training step, stated once: what otal_step_gate decides and what otal_adam_flat_guard
then does, in numpy.  No torch, no device use.

Stock torch leaves a bad step out with GradScaler: `optimizer.step()` is not called when the unscaled gradient holds an inf or
a NaN.  Here the decision is taken on the device, from the value otal_grad_norm left there:

    a step is APPLIED iff the float32 norm out[0] is finite, otherwise it is SKIPPED.

The norm is non-finite whenever an element of the gradient is -- and, deliberately, also for a gradient of finite elements
whose norm overflows float32 (above ~3.4e38): such a step is skipped as well; no update of any use starts from it.

A skipped step changes none of p, m, v, ema, the applied-step count t, nor the criterion's cross-step loss state (it is put
back from the copy the last applied step left); it increments `nonfinite`.  An applied step increments t and runs Adam with
the bias corrections {1 - beta1^t, sqrt(1 - beta2^t)} of the APPLIED count, from the float64 recurrence

    pow1 *= beta1; pow2 *= beta2          (pow = 1.0 at t = 0, the betas rounded to float32 first, as the C entries get them)

then 1 - pow1 and sqrt(1 - pow2) in float64, each rounded to float32 once.  Only IEEE multiply, subtract and sqrt are
involved, so the device reproduces the host bit for bit; for the betas in use the pair equals ops.adam_bias_corrections' (a
pow() call) at every t the tests reach, so a guarded run without a skipped step is bit-identical to an unguarded one.

The host's step count stays "steps run" (applied + skipped): it positions the learning-rate schedule and the EMA warm-up, as
torch's scheduler.step() does whether or not the optimizer stepped.

The device record (OTAL_STEP_GUARD_BYTES = 64, 8-byte aligned) is RECORD below.
"""
import math

import numpy as np

F32 = np.float32
BYTES = 64                                          # OTAL_STEP_GUARD_BYTES
MAX_STATE = 4096                                    # OTAL_STEP_GATE_MAX_STATE: floats of loss state one gate launch copies
RECORD = np.dtype([('applied', '<i8'), ('nonfinite', '<i8'), ('pow1', '<f8'), ('pow2', '<f8'), ('apply', '<i4'),
                   ('reserved', '<i4', (7,))])
assert RECORD.itemsize == BYTES
CHECKPOINT_KEY = 'step_guard'                       # of the train-state file: {'applied': int, 'nonfinite': int}


def bias_powers(t, beta1, beta2):
    """(beta1^t, beta2^t) by the recurrence, float64: t multiplications each, starting at 1.0."""
    t = int(t)
    if t < 0:
        raise ValueError("step guard: the applied-step count cannot be negative")
    b1, b2 = np.float64(F32(beta1)), np.float64(F32(beta2))
    p1, p2 = np.float64(1.0), np.float64(1.0)
    for _ in range(t):
        p1 = p1 * b1
        p2 = p2 * b2
    return p1, p2


def corrections(pow1, pow2):
    """float32 {1 - pow1, sqrt(1 - pow2)}: float64 arithmetic, one rounding each."""
    return F32(np.float64(1.0) - np.float64(pow1)), F32(math.sqrt(np.float64(1.0) - np.float64(pow2)))


def new_record(applied=0, nonfinite=0, beta1=0.9, beta2=0.999):
    """A record (numpy scalar array of dtype RECORD, shape ()) after `applied` applied and `nonfinite` skipped steps."""
    applied, nonfinite = int(applied), int(nonfinite)
    if applied < 0 or nonfinite < 0:
        raise ValueError("step guard: counts cannot be negative")
    r = np.zeros((), dtype=RECORD)
    r['applied'], r['nonfinite'] = applied, nonfinite
    r['pow1'], r['pow2'] = bias_powers(applied, beta1, beta2)
    return r


def gate(norm, record, beta1=0.9, beta2=0.999, host_state=None, loss_state=None, loss_state_keep=None):
    """One otal_step_gate launch.  -> (apply, record') and, with any of the optional arrays, (apply, record', step_state,
    loss_state', loss_state_keep'): step_state the 4 float32 {1 - pow1', sqrt(1 - pow2'), host_state[2] or 1, host_state[3] or
    0}; applied: keep' = state, skipped: state' = keep.  Nothing is modified in place."""
    norm = F32(norm)
    apply = bool(np.isfinite(norm))
    r = np.array(record, dtype=RECORD)
    if apply:
        r['applied'] += 1
        r['pow1'] = np.float64(r['pow1']) * np.float64(F32(beta1))
        r['pow2'] = np.float64(r['pow2']) * np.float64(F32(beta2))
    else:
        r['nonfinite'] += 1
    r['apply'] = int(apply)
    if host_state is None and loss_state is None and loss_state_keep is None:
        return apply, r
    bc = corrections(r['pow1'], r['pow2'])
    step_state = np.asarray([bc[0], bc[1], F32(1.0) if host_state is None else F32(host_state[2]),
                             F32(0.0) if host_state is None else F32(host_state[3])], dtype=F32)
    state = None if loss_state is None else np.array(loss_state, dtype=F32)
    keep = None if loss_state_keep is None else np.array(loss_state_keep, dtype=F32)
    if state is not None and state.size:
        if keep is None:
            raise ValueError("step guard: a loss state needs its keep buffer")
        if apply:
            keep[:state.size] = state
        else:
            state[:] = keep[:state.size]
    return apply, r, step_state, state, keep


def guarded_adam_reference(adam, steps, p, m, v, beta1=0.9, beta2=0.999, record=None, **kw):
    """Run the gradients `steps` (a list of arrays) through `adam(p, g, m, v, beta1=, beta2=, bias_corr=, **kw) -> (p, m, v)`
    -- grad_norm_cases.adam32's signature -- and omit the skipped ones, as common/grad_clip.adam_clip_reference states clipping:
    the norm of each gradient decides (grad_clip.grad_norm_reference at grad_scale kw['grad_scale'] or 1), an applied step gets
    the corrections of the applied count.  -> (p, m, v, record)."""
    from .grad_clip import grad_norm_reference
    r = new_record(0, 0, beta1, beta2) if record is None else record
    for g in steps:
        norm, _ = grad_norm_reference(g, kw.get('grad_scale', 1.0), 0.0)
        apply, r = gate(norm, r, beta1, beta2)
        if apply:
            p, m, v = adam(p, g, m, v, beta1=beta1, beta2=beta2, bias_corr=corrections(r['pow1'], r['pow2']), **kw)
    return p, m, v, r


# ---- checkpoints: what the train-state file holds and what a resume makes of it
def checkpoint_entry(applied, nonfinite):
    return {'applied': int(applied), 'nonfinite': int(nonfinite)}


def counts_from_checkpoint(train_state, step):
    """(applied, nonfinite) of a train-state dict whose optimizer state says `step`; a file without the key is an unguarded
    run's: every step was applied."""
    d = train_state.get(CHECKPOINT_KEY) if hasattr(train_state, 'get') else None
    if d is None:
        return int(step), 0
    applied, nonfinite = int(d['applied']), int(d['nonfinite'])
    if applied < 0 or nonfinite < 0:
        raise ValueError("step guard: the checkpoint holds a negative count")
    return applied, nonfinite


# ---- the drivers' two flags
GUARD_FLAGS = {'skip_nonfinite': False, 'max_nonfinite': None}


def take_guard_flag(argv, i, extra):
    """`--skip_nonfinite` / `--max_nonfinite N` (a whole number >= 0) at argv[i]: `extra` updated, -> the index of the flag's
    last word; any other word -> None.  What the two mean together: check_guard_flags."""
    a = argv[i]
    if a == '--skip_nonfinite':
        extra['skip_nonfinite'] = True
        return i
    if a != '--max_nonfinite':
        return None
    text = argv[i + 1] if i + 1 < len(argv) else None
    try:
        n = int(text)
    except (TypeError, ValueError):
        n = -1
    if n < 0:
        raise SystemExit(f"--max_nonfinite takes a whole number >= 0 (skipped steps the run may log before it ends), not {text!r}")
    extra['max_nonfinite'] = n
    return i + 1


def check_guard_flags(extra):
    if extra.get('max_nonfinite') is not None and not extra.get('skip_nonfinite'):
        raise SystemExit("--max_nonfinite belongs to --skip_nonfinite (without it no step is skipped, and none is counted)")


def limit_message(count, limit):
    return (f"{int(count)} steps had a non-finite gradient and were skipped, more than --max_nonfinite {int(limit)} allows: "
            "ending the run")


def check_limit(count, limit):
    """The drivers' stop rule: SystemExit (a non-zero exit) once the count of skipped steps exceeds `limit` (None: no limit)."""
    if limit is not None and count is not None and int(count) > int(limit):
        raise SystemExit(limit_message(count, limit))
