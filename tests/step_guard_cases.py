"""Cases shared by test_step_guard_cpu.py and test_step_guard_gpu.py: the beta pairs, the norms at the decision's edges, the
eight-step gradient list with four bad steps, and the record's bytes.

Nothing here has a tolerance of its own: the gate, the record and the bias corrections are compared bit for bit (IEEE multiply,
subtract, sqrt and copies); the Adam trajectory borrows the bound of the existing Adam tests (test_grad_norm_cpu.py: within
2 x 2^-24 x e of oracle.head_ref.adam's float64 statement, e its running error)."""
import numpy as np

from opental_amd.common import step_guard as G

F32 = np.float32
BETAS = ((0.9, 0.999), (0.5, 0.9), (0.95, 0.98))
FLT_MAX = F32(np.finfo(np.float32).max)
FINITE_NORMS = (F32(0.0), F32(1.5), FLT_MAX)
BAD_NORMS = (F32(np.inf), F32(-np.inf), F32(np.nan))
NORMS = FINITE_NORMS + BAD_NORMS
STATE_SIZES = (0, 1, 50, 64, 65, G.MAX_STATE)
BAD_STEPS = {1: np.inf, 4: np.nan, 5: -np.inf, 8: np.nan}      # 1-based: a skip before any applied step ... a skip as the last
N_STEPS = 8


def eight_steps(n, where=0, seed=0):
    """Eight float32 gradients of n elements; steps 1, 4, 5 and 8 carry an inf or a NaN at index `where`."""
    rs = np.random.RandomState(seed + n % 983)
    steps = []
    for k in range(1, N_STEPS + 1):
        g = rs.randn(n).astype(F32)
        if k in BAD_STEPS:
            g[where] = F32(BAD_STEPS[k])
        steps.append(g)
    return steps


def finite_steps(steps):
    return [g for g in steps if np.isfinite(g).all()]


def record_bytes(r):
    return np.frombuffer(np.asarray(r, dtype=G.RECORD).tobytes(), dtype=np.int64).copy()


def record_from_bytes(words):
    return np.frombuffer(np.ascontiguousarray(words, dtype=np.int64).tobytes(), dtype=G.RECORD)[0]


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=F32)).view(np.int32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def state_pair(n, seed=0):
    """(loss_state, loss_state_keep) of n floats that differ everywhere, with a NaN and an inf among them when there is room:
    the copy must carry any bits."""
    rs = np.random.RandomState(seed + n)
    a, b = rs.rand(n).astype(F32) + F32(1.0), rs.rand(n).astype(F32) + F32(3.0)
    if n > 2:
        a[1], b[2] = F32(np.nan), F32(np.inf)
    return a, b
