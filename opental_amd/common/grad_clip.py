"""The global-norm rule of the training step, stated once: what otal_grad_norm and otal_adam_flat_clip compute, in numpy.

Reference: `get_grad_norm(net)` written to TensorBoard as `stats/grad_norm` after every backward() and the (disabled)
`nn.utils.clip_grad_norm_(get_trainable_params(net), 20)` beside it, AFSD/thumos14/train.py:134-141,:248-250.

The norm is the L2 norm over every trainable element of the gradient the optimizer sees (the sum over the ranks times
grad_scale = 1 / world), summed in float64 from the float32 values and rounded to float32 once.  The coefficient is
torch.nn.utils.clip_grad_norm_'s, in its float32 arithmetic: `max_norm / (total_norm + 1e-6)` with a Python number on the
left is Tensor.__rtruediv__, i.e. reciprocal() * max_norm (two roundings, not one division), then clamp(max=1.0), which
keeps a NaN.  Adam then reads (g * grad_scale) * coef where it read g * grad_scale.
"""
import numpy as np

F32 = np.float32


def clip_coefficient(norm, max_norm):
    """float32 coefficient for a float32 `norm`; max_norm None or <= 0: no clipping, 1."""
    if max_norm is None or max_norm <= 0:
        return F32(1.0)
    with np.errstate(all="ignore"):
        c = F32(F32(1.0) / F32(F32(norm) + F32(1e-6))) * F32(max_norm)
    return F32(1.0) if c >= F32(1.0) else F32(c)        # (a NaN compares false and stays)


def grad_norm_reference(g, grad_scale=1.0, max_norm=0.0):
    """-> (norm, coef), both numpy float32, of the float32 values `g` (any shape; numpy array or CPU/GPU tensor)."""
    if hasattr(g, "detach"):
        g = g.detach().cpu().numpy()
    g = np.asarray(g, dtype=F32).reshape(-1).astype(np.float64)
    with np.errstate(all="ignore"):
        norm = F32(np.sqrt(np.sum(g * g)) * float(F32(grad_scale)))
    return norm, clip_coefficient(norm, max_norm)


def prescale(g, grad_scale, coef):
    """The gradient Adam's arithmetic starts from under clipping: float32 (g * grad_scale) * coef, rounded after each
    product as the kernel does."""
    g = np.asarray(g, dtype=F32)
    with np.errstate(all="ignore"):
        return (g * F32(grad_scale)).astype(F32) * F32(coef)


def adam_clip_reference(adam, p, g, m, v, grad_scale, coef, **kw):
    """The clipped update in its pre-scaled form: `adam(p, g', m, v, grad_scale=1.0, **kw)` on g' = prescale(g, grad_scale,
    coef).  `adam` is any statement of torch.optim.Adam's single-tensor update with that signature; multiplying g' by 1.0
    is exact, so it continues the kernel's arithmetic at `gi + wd * p`."""
    return adam(p, prescale(g, grad_scale, coef), m, v, grad_scale=1.0, **kw)
