"""The learning-rate schedule and the weight EMA of the training step, stated once: what the host writes into the step's
device record and what otal_adam_flat_sched computes from it, in numpy.  No device use.

The schedule is a MULTIPLIER of every optimizer group's base rate, a function of the 1-based optimisation step `t` about to
run (torch.optim.lr_scheduler's chainable forms, stepped once per optimisation step, evaluated in closed form):

    warm-up, t <= W:                 t / W                                  (LinearLR(start_factor=1/W, total_iters=W-1))
    behind it, tau = clamp((t - W - 1) / max(1, T - W - 1), 0, 1):
        constant                     1
        cosine                       r + (1 - r) * 0.5 * (1 + cos(pi * tau))          (CosineAnnealingLR(T - W - 1, eta_min = r * lr))
        multistep                    gamma ** #{M in milestones : t > M}              (MultiStepLR, milestones in steps)
    t > T                            the value at T

What the device sees is s32 = float32(multiplier); a group's effective rate is the float32 product float32(group_lr) * s32
(`effective_lr32`), formed once per thread by the kernel -- and once on the host by whoever wants the same bits from
otal_adam_flat_dev.

The averaged model: ema' = ema + (p' - ema) * (1 - keep) with p' the parameter AFTER the step's update and
keep = float32(min(decay, (1 + t) / (10 + t))): the ramp lets randomly initialised heads leave their initial values quickly,
and is why the factor is a per-step device scalar and not a launch constant.
"""
import math

import numpy as np

F32 = np.float32
NAMES = ('constant', 'cosine', 'multistep')


def check(name, total_steps, warmup_steps=0, min_lr_ratio=0.0, milestones=(), gamma=0.1):
    """The arguments of `multiplier`, normalised -> (name, T, W, r, milestones, gamma); ValueError for what has no meaning."""
    if name not in NAMES:
        raise ValueError("lr schedule: %r is not one of %s" % (name, ", ".join(NAMES)))
    T, W = int(total_steps), int(warmup_steps)
    if T != total_steps or W != warmup_steps or T < 1 or W < 0:
        raise ValueError("lr schedule: total_steps must be a whole number >= 1 and warmup_steps one >= 0")
    if W >= T:
        raise ValueError("lr schedule: warmup_steps (%d) must be smaller than total_steps (%d)" % (W, T))
    r = float(min_lr_ratio)
    if not 0.0 <= r <= 1.0:
        raise ValueError("lr schedule: min_lr_ratio must lie in [0, 1]")
    ms = tuple(int(m) for m in milestones)
    if any(b <= a for a, b in zip(ms, ms[1:])) or any(m != m0 for m, m0 in zip(ms, milestones)):
        raise ValueError("lr schedule: milestones must be increasing whole numbers of steps")
    g = float(gamma)
    if not math.isfinite(g) or g < 0.0:
        raise ValueError("lr schedule: gamma must be a finite number >= 0")
    return name, T, W, r, ms, g


def multiplier(name, t, total_steps, warmup_steps=0, min_lr_ratio=0.0, milestones=(), gamma=0.1):
    """float64 multiplier of the base rates at the 1-based step `t`."""
    name, T, W, r, ms, g = check(name, total_steps, warmup_steps, min_lr_ratio, milestones, gamma)
    t = int(t)
    if t < 1:
        raise ValueError("lr schedule: steps are counted from 1")
    t = min(t, T)                                       # behind the last step: its value
    if t <= W:
        return np.float64(t) / np.float64(W)
    if name == 'constant':
        return np.float64(1.0)
    if name == 'cosine':
        tau = min(max((t - W - 1) / max(1, T - W - 1), 0.0), 1.0)
        return np.float64(r + (1.0 - r) * 0.5 * (1.0 + math.cos(math.pi * tau)))
    return np.float64(g) ** sum(1 for m in ms if t > m)


def effective_lr32(group_lr, s):
    """The rate the kernel's arithmetic runs at: float32(group_lr) * float32(s), one float32 product."""
    return F32(F32(group_lr) * F32(s))


def ema_keep(decay, t):
    """float32 keep factor of the EMA at the 1-based step t: min(decay, (1 + t) / (10 + t))."""
    d = float(decay)
    if not 0.0 <= d < 1.0:
        raise ValueError("ema decay must lie in [0, 1)")
    t = int(t)
    if t < 1:
        raise ValueError("ema: steps are counted from 1")
    return F32(min(d, (1.0 + t) / (10.0 + t)))


def step_state(bias_corr, s=1.0, keep=0.0):
    """The four floats of the device record: {1 - b1^t, sqrt(1 - b2^t), lr multiplier, ema keep factor}."""
    return np.asarray([bias_corr[0], bias_corr[1], F32(s), F32(keep)], dtype=F32)


def ema_reference(ema, p_new, keep):
    """float64 ema + (float32(p' - ema)) * (1 - keep): the difference rounded to float32 as the kernel rounds it, 1 - keep the
    kernel's float32 scalar, everything behind in float64 -- the kernel's fmaf rounds that ONCE, so its result is the
    float32 nearest to this value, or (double rounding when this value is then rounded again) its neighbour."""
    ema, p_new = np.asarray(ema, dtype=F32), np.asarray(p_new, dtype=F32)
    drop = np.float64(F32(1.0) - F32(keep))
    with np.errstate(all="ignore"):
        d = (p_new - ema).astype(F32).astype(np.float64)
        return ema.astype(np.float64) + d * drop


def adam_sched_reference(adam, p, g, m, v, grad_scale, lr, s=1.0, coef=None, ema=None, keep=None, **kw):
    """The scheduled update in float64: `adam` (oracle.head_ref.adam's signature, as grad_clip.adam_clip_reference takes it) at
    the effective rate effective_lr32(lr, s), on the clipped gradient when `coef` is given, plus -- `ema` given -- the EMA of
    the NEW parameter.  -> (p, e_p), (m, e_m), (v, e_v)[, (ema, e_ema)]: each result with its running error bound in units
    of one float32 rounding, the form `adam` returns (K = 1 in the tests' bound).

    The EMA's bound continues p's: d = p' - ema carries e_p + |d|, the product with the float32 scalar 1 - keep scales it
    (+ |t| for a rounding the fmaf does not even make), the sum adds |ema'|."""
    rate = effective_lr32(lr, s)
    if coef is None:
        out = adam(p, g, m, v, lr=rate, grad_scale=grad_scale, **kw)
    else:
        from .grad_clip import adam_clip_reference
        out = adam_clip_reference(adam, p, g, m, v, grad_scale, coef, lr=rate, **kw)
    if ema is None:
        return out
    (pn, ep) = out[0]
    e0 = np.asarray(ema, dtype=F32).astype(np.float64)
    drop = float(F32(1.0) - F32(keep))
    d = pn - e0; ed = ep + np.abs(d)
    t = d * drop; et = ed * drop + np.abs(t)
    en = e0 + t; een = et + np.abs(en)
    return out[0], out[1], out[2], (en, een)
