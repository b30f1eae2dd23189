"""Cases shared by test_lr_schedule_cpu.py and test_lr_schedule_gpu.py: the schedule grid, the kernel's sizes and
alignments, dyadic inputs on which the EMA line is exact, and the one-ulp comparison of arrays.

Tolerances (derived, not measured):
 * multiplier against torch's schedulers: relative 1e-12 in float64.  torch's chainable forms reach the value of step t by t
   recursive float64 updates, each within 2^-53 relatively; at T <= 50 that is below 1e-14, and the cosine near its floor
   loses a few digits to cancellation in (1 + cos) -- 1e-12 leaves room for both and is far below one float32 ulp (6e-8),
   which is all the device ever sees of the multiplier.
 * the EMA line: the kernel rounds d = p' - ema once and fmaf(d, 1 - keep, ema) once; the rule (lr_schedule.ema_reference)
   rounds the same d in float32 and does the rest in float64, where the product of two float32 values is exact and the sum is
   within 2^-53.  Rounding that float64 value to float32 differs from the fmaf's single rounding only when the float64 value
   sits within 2^-53 (relative) of a float32 rounding boundary: the results are then neighbours.  Hence: within ONE float32
   ulp, and the same bits on dyadic inputs where d, the product and the sum are all exact.
"""
import numpy as np

F32 = np.float32
TOTALS, WARMUPS = (2, 7, 50), (0, 1, 3)
GRID = [(T, W) for T in TOTALS for W in WARMUPS if W < T]
REFUSED = [(T, W) for T in TOTALS for W in WARMUPS if W >= T]
REL = 1e-12
# (p, g, m, v, ema) offsets in floats into the guarded buffers: 4 = 16-byte aligned
ALIGNMENTS = {"aligned": (4, 4, 4, 4, 4), "ema+1": (4, 4, 4, 4, 5), "p+1": (5, 4, 4, 4, 4)}
EXTRA_SIZE = 4 * 256 + 1


def sizes(grad_norm_sizes):
    """GC.SIZES without its largest entry (no grid cap beyond the existing rule is involved), plus 4 * 256 + 1."""
    return tuple(dict.fromkeys(tuple(grad_norm_sizes[:-1]) + (EXTRA_SIZE,)))


def ema_state(n, seed=0):
    rs = np.random.RandomState(seed + n % 983)
    return (rs.randn(n) * 0.7).astype(F32)


def dyadic_state(n, seed=0):
    """(p, g, m, v, ema) with g = m = v = 0, weight decay 0 assumed: Adam leaves p as it is (the update is 0 / eps-only
    denominators times 0), p and ema small multiples of 2^-6 -- p - ema, its half and the sum with ema are exact."""
    rs = np.random.RandomState(seed + n % 971)
    p = (rs.randint(-64, 65, n).astype(F32) * F32(2.0 ** -6)).astype(F32)
    e = (rs.randint(-64, 65, n).astype(F32) * F32(2.0 ** -6)).astype(F32)
    z = np.zeros(n, dtype=F32)
    return p, z.copy(), z.copy(), z.copy(), e


def ulp_distance(a, b):
    """Per element: how many float32 values apart (0 = same bits; NaN pairs count as 0, a NaN against a number as huge)."""
    a, b = np.ascontiguousarray(a, dtype=F32), np.ascontiguousarray(b, dtype=F32)
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, np.int64(-2 ** 31) - ia, ia)          # sign-magnitude -> a monotone integer line
    ib = np.where(ib < 0, np.int64(-2 ** 31) - ib, ib)
    d = np.abs(ia - ib)
    both_nan = np.isnan(a) & np.isnan(b)
    one_nan = np.isnan(a) ^ np.isnan(b)
    return np.where(both_nan, 0, np.where(one_nan, np.int64(2 ** 40), d))


def within_one_ulp(a, b):
    return bool((ulp_distance(a, b) <= 1).all())
