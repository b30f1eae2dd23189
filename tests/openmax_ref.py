"""Helper of tests/test_openmax_{cpu,gpu}.py and tools/pin_openmax.py (not a test module): the seeded synthetic inputs of
the OpenMax fixture and numpy restatements of what the reference computes (AFSD/thumos14/openmax.py, test_openmax.py, libMR).

  * inputs     -- regenerated from np.random.RandomState seeds stored in tests/golden/openmax.npz, so the fixture keeps only
                  MAVs, tails, parameters and reference outputs;
  * float64    -- eucos / w_score / recalibrate / decode in float64: must equal the golden (which the reference produced in
                  float64 from float32-valued inputs) to rtol 1e-9 -- this pins the checker;
  * float32    -- the same arithmetic in plain float32 numpy with the stable w-score form: its deviation from the reference
                  is what the pin tool records as the yardstick of the GPU tolerances (the tests allow 4x);
  * exact MLE  -- the Weibull likelihood equation solved in extended precision by bisection, independent of the package.
"""
import numpy as np

K, D, A = 15, 512, 126
TRANSLATE = 10000.0
LEVELS = (64, 32, 16, 8, 4, 2)


# ----------------------------------------------------------------------------- seeded inputs
def class_centres(seed, k=K, d=D):
    """Non-negative class centres, like ReLU tower outputs."""
    return np.abs(np.random.RandomState(seed).normal(0.0, 1.0, (k, d))).astype(np.float32)


def features_of(centres, labels, seed):
    """Rows clustered round the centre of their class, non-negative; the per-row spread varies so that the distances to the
    class mean span both sides of a fitted tail."""
    rs = np.random.RandomState(seed)
    spread = rs.uniform(0.15, 0.9, (len(labels), 1))
    noise = rs.normal(0.0, 1.0, (len(labels), centres.shape[1]))
    return np.maximum(centres[labels] + spread * noise, 0.0).astype(np.float32)


def stat_labels(per_class=40, k=K):
    """Labels of the statistics rows: `per_class` rows of every class, interleaved."""
    return np.tile(np.arange(k), per_class).astype(np.int64)


def logits_of(labels, seed, boost=3.0, k=K, background=False, sigma=2.0):
    """Logits of a few units that favour the row's own class; with `background` a leading background logit."""
    rs = np.random.RandomState(seed)
    z = rs.normal(0.0, sigma, (len(labels), k + int(background)))
    z[np.arange(len(labels)), labels + int(background)] += boost
    return z.astype(np.float32)


def priors():
    return np.array([[(c + 0.5) / t] for t in LEVELS for c in range(t)], np.float32)


def clip_outputs(seed, centres, prop_centres, n=2):
    """Head outputs + tower features of `n` clips as the closed-set network returns them with get_feat=True.  The logits
    single out one class per anchor, so that a class keeps a few dozen candidates whose scores lie well apart."""
    rs = np.random.RandomState(seed)
    lab = rs.randint(0, K, (n, A))
    out = dict(loc=rs.uniform(2.0, 40.0, (n, A, 2)).astype(np.float32),
               prop_loc=rs.normal(0.0, 0.3, (n, A, 2)).astype(np.float32),
               center=rs.normal(0.0, 1.0, (n, A, 1)).astype(np.float32))
    out['conf'] = logits_of(lab.reshape(-1), seed + 1, boost=7.0, background=True, sigma=1.0).reshape(n, A, K + 1)
    out['prop_conf'] = logits_of(lab.reshape(-1), seed + 2, boost=7.0, background=True, sigma=1.0).reshape(n, A, K + 1)
    out['conf_feat'] = features_of(centres, lab.reshape(-1), seed + 3).reshape(n, A, D)
    out['prop_conf_feat'] = features_of(prop_centres, lab.reshape(-1), seed + 4).reshape(n, A, D)
    return out


def match_inputs(seed, b=3):
    """loc (b, A, 2) and ragged targets for get_matched_targets; the last sample has a ground truth no prior lies in."""
    rs = np.random.RandomState(seed)
    loc = rs.uniform(2.0, 60.0, (b, A, 2)).astype(np.float32)
    targets = [np.array([[0.10, 0.30, 3.0], [0.22, 0.27, 9.0], [0.45, 0.62, 7.0], [0.70, 0.95, 15.0]], np.float32),
               np.array([[0.05, 0.55, 1.0], [0.20, 0.35, 12.0]], np.float32),
               np.array([[0.0, 0.005, 2.0]], np.float32)][:b]
    return loc, targets


# ----------------------------------------------------------------------------- the arithmetic, dtype by dtype
def eucos(mav, feat, dt=np.float64):
    """compute_eucos_dist (openmax.py:7-9) of rows `feat` (N, D) against `mav` (K, D) -> (N, K)."""
    m, f = np.asarray(mav, dt), np.asarray(feat, dt)
    diff = f[:, None, :] - m[None, :, :]
    eu = np.sqrt(np.sum(diff * diff, -1, dtype=dt))
    uv = np.sum(f[:, None, :] * m[None, :, :], -1, dtype=dt)
    uu = np.sum(f * f, -1, dtype=dt)[:, None]
    vv = np.sum(m * m, -1, dtype=dt)[None, :]
    return eu / dt(200) + (dt(1) - uv / (np.sqrt(uu) * np.sqrt(vv)))


def class_mean_f32(feat_rows):
    """A plain float32 mean of (n, D) rows in another summation order than np.mean(axis=0): numpy's pairwise sum along the
    contiguous axis of the transpose."""
    t = np.ascontiguousarray(np.asarray(feat_rows, np.float32).T)
    return (t.sum(axis=1, dtype=np.float32) / np.float32(t.shape[1])).astype(np.float32)


def w_score64(d, scale, shape, small):
    """libMR's w_score (MetaRecognition.cpp:141-152, weibull.c:79-104) in float64."""
    x = np.asarray(d, np.float64) + TRANSLATE - small
    return np.where(x < 0, 0.0, 1.0 - np.exp(-np.power(np.maximum(x, 0.0) / scale, shape)))


def w_constants(scale, shape, small):
    """(off, 1 / scale, shape), formed in float64 (include/opental_hip.h: otal_openmax_probs)."""
    return np.stack([np.asarray(small, np.float64) + (np.asarray(scale, np.float64) - TRANSLATE),
                     1.0 / np.asarray(scale, np.float64), np.asarray(shape, np.float64)], -1)


def w_score32_stable(d, wb):
    """float32: w = -expm1(-exp(shape * log1p((d - off) / scale))), 0 where the translated argument is <= 0."""
    wb = np.asarray(wb, np.float32)
    u = (np.asarray(d, np.float32) - wb[..., 0]) * wb[..., 1]
    with np.errstate(invalid='ignore', divide='ignore'):
        w = -np.expm1(-np.exp(wb[..., 2] * np.log1p(u)))
    return np.where(u <= np.float32(-1), np.float32(0), w).astype(np.float32)


def w_score32_literal(d, scale, shape, small):
    """float32, the formula as libMR writes it (what the kernel must NOT do)."""
    x = np.asarray(d, np.float32) + np.float32(TRANSLATE) - np.asarray(small, np.float32)
    return (np.float32(1) - np.exp(-np.power(x / np.asarray(scale, np.float32), np.asarray(shape, np.float32)))).astype(np.float32)


def recalibrate(logits, dist, w, rank, dt=np.float64):
    """openmax_recalibrate + compute_openmax_prob (openmax.py:21-73) for rows: logits (N, K), w (N, K) w-scores -> (N, K + 1).
    The softmax subtracts the largest exponent (same value)."""
    z = np.asarray(logits, dt)
    n, k = z.shape
    order = np.argsort(z, axis=1)[:, ::-1]
    alpha = np.zeros((n, k), dt)
    for i in range(rank):
        alpha[np.arange(n), order[:, i]] = dt((rank - i) / float(rank))
    mod = z * (dt(1) - np.asarray(w, dt) * alpha)
    unk = np.sum(z - mod, 1, dtype=dt)
    ex = np.concatenate([unk[:, None], mod], 1)
    ex = np.exp(ex - ex.max(1, keepdims=True))
    return (ex / ex.sum(1, keepdims=True, dtype=dt)).astype(dt)


def openmax_probs(logits, feat, mav, fits, rank, dt=np.float64):
    """OpenMax.forward.  fits: dict(scale, shape, small) of (K,) float64 arrays.  float64: libMR's formula; float32: the stable
    form on float64-prepared constants."""
    d = eucos(mav, feat, dt)
    if dt == np.float64:
        w = w_score64(d, fits['scale'], fits['shape'], fits['small'])
    else:
        w = w_score32_stable(d, w_constants(fits['scale'], fits['shape'], fits['small']).astype(np.float32))
    return recalibrate(logits, d, w, rank, dt)


def decode(out, clips, mav, fits, mav_prop, fits_prop, clip_length=256.0, rank=1, refined_feature=False, dt=np.float64):
    """decode_output (test_openmax.py:141-170) per clip: seg (n, A, 2) float32 arithmetic as the reference, score
    (n, K + 1, A) with row 0 = unknown."""
    n = out['loc'].shape[0]
    pri = priors()
    segs, scores = [], []
    for i in range(n):
        loc, ploc = out['loc'][i], out['prop_loc'][i]
        w = loc[:, :1] + loc[:, 1:]
        l2 = np.float32(0.5) * w * ploc + loc
        seg = np.concatenate([pri * np.float32(clip_length) - l2[:, :1], pri * np.float32(clip_length) + l2[:, 1:]], -1)
        seg = np.clip(seg, 0, np.float32(clip_length))
        segs.append(((seg + np.float32(clips[i][0])) / np.float32(clips[i][1])).astype(np.float32))
        feat = out['conf_feat'][i]
        p0 = openmax_probs(out['conf'][i][:, 1:], feat, mav, fits, rank, dt)
        p1 = openmax_probs(out['prop_conf'][i][:, 1:], out['prop_conf_feat'][i] if refined_feature else feat, mav_prop,
                           fits_prop, rank, dt)
        if dt == np.float64:        # the reference's centre factor is torch's float32 sigmoid, promoted
            import torch
            ct = torch.from_numpy(np.ascontiguousarray(out['center'][i])).sigmoid().numpy().astype(np.float64)
        else:
            ct = (np.float32(1) / (np.float32(1) + np.exp(-out['center'][i]))).astype(np.float32)
        scores.append((((p0 + p1) / dt(2)) * ct).T)
    return np.stack(segs), np.stack(scores)


# ----------------------------------------------------------------------------- exact Weibull MLE (extended precision)
def weibull_mle_exact(tail):
    """Maximum-likelihood Weibull (scale, shape) of x = tail + 10000 - min(tail) and small = min(tail): the
    smallest-extreme-value likelihood equation on log x, bisected in np.longdouble until the bracket stops shrinking."""
    ld = np.longdouble
    d = np.sort(np.asarray(tail, np.float64))[::-1]
    small = float(d[-1])
    y = np.log((d + TRANSLATE - small).astype(ld))
    ymax, rng = y.max(), y.max() - y.min()
    y0 = (y - ymax) / rng
    ybar = y0.mean()

    def g(s):
        e = np.exp(y0 / s)
        return s + ybar - (y0 * e).sum() / e.sum()
    lo = hi = ld(np.sqrt(6.0)) * y0.std(ddof=1) / ld(np.pi)
    while g(lo) > 0:
        lo = lo / 2
    while g(hi) < 0:
        hi = hi * 2
    for _ in range(300):
        mid = (lo + hi) / 2
        if mid <= lo or mid >= hi:
            break
        if g(mid) > 0:
            hi = mid
        else:
            lo = mid
    s = (lo + hi) / 2
    mu = s * np.log(np.exp(y0 / s).mean())
    return float(np.exp(rng * mu + ymax)), float(1 / (rng * s)), small
