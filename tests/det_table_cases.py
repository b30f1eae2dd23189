"""Seeded Soft-NMS outputs (rows, counts, durations) for the detection-table tests, CPU and GPU: every way a row can leave
the table is present, and most rows stay."""
import numpy as np

SCORINGS = ('uncertainty', 'confidence', 'uncertainty_actionness', 'a_by_inv_u', 'u_by_inv_a', 'half_au')
SENTINEL = -77


def make_case(V, K, top_k, cols=5, seed=0, counts=None):
    """-> rows (V, K, top_k, cols) float32, counts (V, K) int32, durations (V,) float64.
    Counted rows: a seventh of them, in turn, get a score of 0 / -1 / NaN, a negative start, an end past the duration, a
    segment wholly past the duration, start == end, an end equal to the duration rounded to float32, and a start one float32
    step below the rounded duration with the end past it (the last two separate an fp64 comparison from an fp32 one).
    Rows at and past the count hold valid segments with a score of 1e6: a reader that looks at them is found out.
    counts: the first list has 0 rows, the last top_k, the others top_k - 2 .. top_k (or `counts` for all lists)."""
    rs = np.random.RandomState(seed)
    durations = rs.uniform(20.0, 60.0, V)
    dur = durations[:, None, None]
    start = rs.uniform(0.0, 0.6, (V, K, top_k)) * dur
    rows = np.zeros((V, K, top_k, 5), dtype=np.float64)
    rows[..., 0] = start
    rows[..., 1] = start + rs.uniform(0.5, 0.3 * 20.0, (V, K, top_k))
    rows[..., 2] = rs.uniform(0.01, 1.0, (V, K, top_k))
    rows[..., 3] = rs.uniform(0.05, 0.95, (V, K, top_k))
    rows[..., 4] = rs.uniform(0.5, 1.0, (V, K, top_k))
    rows = rows.astype(np.float32)
    if counts is None:
        cnt = rs.randint(max(0, top_k - 2), top_k + 1, (V, K)).astype(np.int32)
        cnt.flat[0] = 0
        cnt.flat[-1] = top_k
    else:
        cnt = np.full((V, K), counts, dtype=np.int32)
    kind = 0
    for v in range(V):
        d32 = np.float32(durations[v])
        for c in range(K):
            for i in range(int(cnt[v, c])):
                if (v * K * top_k + c * top_k + i) % 7 != 3:
                    continue
                r = rows[v, c, i]
                m = kind % 9
                kind += 1
                if m == 0:
                    r[2] = 0.0
                elif m == 1:
                    r[2] = -1.0
                elif m == 2:
                    r[2] = np.nan
                elif m == 3:
                    r[0] = -3.5
                elif m == 4:
                    r[1] = durations[v] + 5.0
                elif m == 5:
                    r[0], r[1] = durations[v] + 1.0, durations[v] + 4.0
                elif m == 6:
                    r[1] = r[0]
                elif m == 7:
                    r[1] = d32
                else:
                    r[0], r[1] = np.nextafter(d32, np.float32(0.0)), durations[v] + 3.0
            rows[v, c, int(cnt[v, c]):, 2] = 1e6
    return np.ascontiguousarray(rows[..., :cols]), cnt, durations
