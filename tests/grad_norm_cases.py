"""Cases shared by test_grad_norm_cpu.py and test_grad_norm_gpu.py: the sizes and inputs of the global-norm launch, a float32
restatement of the flat Adam's arithmetic (csrc/misc.hip adam_one; the oracle's own statement is oracle/head_ref.adam), and
the one-ulp comparison.

Tolerance of the norm (derived, not measured): the squares of float32 values are exact in float64, the kernel adds them
in float64 in a fixed order, numpy in its pairwise order; either sum of n <= 2^26 non-negative terms is within n * 2^-53
of the exact one, relatively, the square root halves that, and the one rounding to float32 is within 2^-24.  Two values
that each sit within (2^-25 + 2^-27) of the exact result are at most ONE float32 ulp apart; on inputs whose squares sum
exactly (small integers times a power of two) both sums are the exact one and the bits must agree."""
import numpy as np

F32 = np.float32
GRID_CAP = 2048                                     # OTAL_GRAD_NORM_PARTIALS: blocks of 256 threads, four elements per trip
SIZES = (1, 3, 4, 5, 255, 256, 257, 1023, 4 * 256 + 1, GRID_CAP * 256 * 4 + 5)   # the last: one full sweep + a ragged tail
KINDS = ("randn", "exact", "zeros", "big", "denormal", "inf", "nan")


def make_input(kind, n, seed=0):
    rs = np.random.RandomState(seed + n % 977)
    if kind == "randn":
        return rs.randn(n).astype(F32)
    if kind == "exact":                             # |k| <= 8 times 2^-3: every square and every partial sum is exact in float64
        return (rs.randint(-8, 9, n).astype(F32) * F32(0.125)).astype(F32)
    if kind == "zeros":
        return np.zeros(n, dtype=F32)
    g = (rs.randn(n) * 0.01).astype(F32)
    j = int(rs.randint(0, n))
    if kind == "big":                               # 1e36 as a float32 square is inf; in float64 it is not
        g[j] = F32(1e18)
    elif kind == "denormal":
        g = (rs.randint(-1000, 1001, n).astype(np.float64) * 2.0 ** -149).astype(F32)     # multiples of the smallest denormal
        g[j] = F32(2.0 ** -140)
    elif kind == "inf":
        g[j] = F32(-np.inf)
    elif kind == "nan":
        g[j] = F32(np.nan)
    else:
        raise ValueError(kind)
    return g


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=F32)).view(np.int32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def within_one_ulp(a, b):
    """Two float32 scalars: equal bits (NaN with NaN, inf with the same inf), or finite neighbours."""
    a, b = F32(a), F32(b)
    if np.isnan(a) or np.isnan(b):
        return bool(np.isnan(a) and np.isnan(b))
    if np.isinf(a) or np.isinf(b):
        return bool(a == b)
    ia, ib = int(bits(a).reshape(-1)[0]), int(bits(b).reshape(-1)[0])
    return (ia >= 0) == (ib >= 0) and abs(ia - ib) <= 1 or (a == 0 and b == 0)


def adam32(p, g, m, v, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, bias_corr=(1.0, 1.0), grad_scale=1.0):
    """adam_one (csrc/misc.hip) in numpy float32, operation by operation and without contraction -- the arithmetic of
    torch.optim.Adam's single-tensor path that the existing Adam oracle states in float64 with its error terms.
    -> (p, m, v) float32."""
    p, g, m, v = (np.asarray(a, dtype=F32) for a in (p, g, m, v))
    lr, b1, b2, eps, wd, gs = (F32(s) for s in (lr, beta1, beta2, eps, weight_decay, grad_scale))
    bc1, bc2s = F32(bias_corr[0]), F32(bias_corr[1])
    one = F32(1.0)
    with np.errstate(all="ignore"):
        gi = g * gs
        gi = gi + wd * p
        mi = m + (gi - m) * (one - b1)
        vi = v * b2 + (one - b2) * gi * gi
        denom = np.sqrt(vi) / bc2s + eps
        pn = p - (lr / bc1) * (mi / denom)
    return pn.astype(F32), mi.astype(F32), vi.astype(F32)


def adam_state(n, seed=0):
    """p, g, m, v of a step > 1, with a few elements that have nothing to move."""
    rs = np.random.RandomState(seed + n % 991)
    p, g = rs.randn(n).astype(F32), rs.randn(n).astype(F32)
    m, v = (rs.randn(n) * 0.1).astype(F32), (rs.randn(n) ** 2 * 0.01).astype(F32)
    g[::97] = 0.0
    m[::97], v[::97] = 0.0, 0.0
    return p, g, m, v
