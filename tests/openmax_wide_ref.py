"""Helper of tests/test_openmax_wide_{cpu,gpu}.py and tools/pin_openmax_wide.py (not a test module): the seeded synthetic
inputs of the K = 150 OpenMax fixture (tests/golden/openmax_wide.npz) and the decode restatement with the ActivityNet priors.
The generators and the arithmetic (eucos, w-scores, recalibrate, openmax_probs) are those of tests/openmax_ref.py, called
with k = 150; only what that file ties to the THUMOS14 layout (126 anchors, (A, 1) priors, 256-frame clips) is restated here.

MAVs are the seeded class centres THEMSELVES (not means of rows), so the fixture stores no 600 KB of MAVs.
"""
import numpy as np

import openmax_ref as R

K, D, A = 150, 512, 189
LEVELS = (96, 48, 24, 12, 6, 3)                 # the ActivityNet pyramid at 768 frames (anet/BDNet.py:262-269)
CLIP_LENGTH = 768.0
NAMES = [f"class_{i}" for i in range(1, K + 1)]
PER_CLASS, TAILSIZE = 40, 20
DECODE_ANCHORS = np.arange(0, A, 3)             # the anchors whose float64 scores the fixture stores (every level is hit)


def priors():
    """(189, 2): centre and level id, as the ActivityNet model returns them."""
    return np.array([[(c + 0.5) / t, i] for i, t in enumerate(LEVELS) for c in range(t)], np.float32)


def mavs(fx):
    return R.class_centres(int(fx["seed_centres"]), K, D), R.class_centres(int(fx["seed_prop_centres"]), K, D)


def fits_of(fx, stage):
    p = fx["fit_params"][stage * K:(stage + 1) * K]
    return dict(scale=p[:, 0], shape=p[:, 1], small=p[:, 2])


def stat_rows(centres, seed):
    """PER_CLASS labelled rows of every class round its centre -> (feat (K * PER_CLASS, D), labels)."""
    labels = R.stat_labels(PER_CLASS, K)
    return R.features_of(centres, labels, seed), labels


def eucos_own(mav_rows, feat, dt=np.float64):
    """compute_eucos_dist (openmax.py:7-9) of row n of `feat` against row n of `mav_rows` -> (N,)."""
    m, f = np.asarray(mav_rows, dt), np.asarray(feat, dt)
    diff = f - m
    eu = np.sqrt(np.sum(diff * diff, -1, dtype=dt))
    uv, uu, vv = np.sum(f * m, -1, dtype=dt), np.sum(f * f, -1, dtype=dt), np.sum(m * m, -1, dtype=dt)
    return eu / dt(200) + (dt(1) - uv / (np.sqrt(uu) * np.sqrt(vv)))


def tails_of(dist, labels):
    """The TAILSIZE largest float32-rounded distances of every class, ascending -> (K, TAILSIZE) float64."""
    d = np.asarray(dist, np.float32).astype(np.float64)
    return np.stack([np.sort(d[labels == k])[-TAILSIZE:] for k in range(K)])


def fit_grid(tail):
    """41 points from a quarter span below the tail to a quarter span above it (the grid of tools/pin_openmax.py)."""
    span = tail.max() - tail.min()
    return np.linspace(tail.min() - 0.25 * span, tail.max() + 0.25 * span, 41)


def prob_rows(fx, n=64):
    seed = int(fx["seed_rows"])
    lab = np.random.RandomState(seed).randint(0, K, n)
    return R.features_of(mavs(fx)[0], lab, seed + 1), R.logits_of(lab, seed + 2, k=K), lab


def clip_outputs(seed, centres, prop_centres, n=2):
    """Head outputs + tower features of `n` ActivityNet clips as the closed-set network returns them with get_feat=True:
    151 logits per anchor (class 0 = background), loc in frames."""
    rs = np.random.RandomState(seed)
    lab = rs.randint(0, K, (n, A))
    out = dict(loc=rs.uniform(2.0, 200.0, (n, A, 2)).astype(np.float32),
               prop_loc=rs.normal(0.0, 0.3, (n, A, 2)).astype(np.float32),
               center=rs.normal(0.0, 1.0, (n, A, 1)).astype(np.float32))
    flat = lab.reshape(-1)
    out['conf'] = R.logits_of(flat, seed + 1, boost=7.0, k=K, background=True, sigma=1.0).reshape(n, A, K + 1)
    out['prop_conf'] = R.logits_of(flat, seed + 2, boost=7.0, k=K, background=True, sigma=1.0).reshape(n, A, K + 1)
    out['conf_feat'] = R.features_of(centres, flat, seed + 3).reshape(n, A, D)
    out['prop_conf_feat'] = R.features_of(prop_centres, flat, seed + 4).reshape(n, A, D)
    return out


def segments(out, clips, clip_length=CLIP_LENGTH):
    """anet/test.py:110-115 in float32, then (segment + offset) / fps as its `filtering` does -> (n, A, 2) float32."""
    pri = priors()[:, :1]
    segs = []
    for i in range(out['loc'].shape[0]):
        loc, ploc = out['loc'][i], out['prop_loc'][i]
        w = loc[:, :1] + loc[:, 1:]
        l2 = np.float32(0.5) * w * ploc + loc
        seg = np.concatenate([pri * np.float32(clip_length) - l2[:, :1], pri * np.float32(clip_length) + l2[:, 1:]], -1)
        seg = np.clip(seg, 0, np.float32(clip_length))
        segs.append(((seg + np.float32(clips[i][0])) / np.float32(clips[i][1])).astype(np.float32))
    return np.stack(segs)


def centre_factor(center, dt):
    if dt == np.float64:            # the reference's centre factor is torch's float32 sigmoid, promoted
        import torch
        return torch.from_numpy(np.ascontiguousarray(center)).sigmoid().numpy().astype(np.float64)
    return (np.float32(1) / (np.float32(1) + np.exp(-center))).astype(np.float32)


def decode(out, mav, fits, mav_prop, fits_prop, rank=1, refined_feature=False, dt=np.float64):
    """The score arithmetic of decode_output (thumos14/test_openmax.py:158-164) per clip on K = 150 classes -> (n, K + 1, A),
    row 0 = unknown.  As shipped the refined stage's layer reads the COARSE feature; refined_feature reads the refined one."""
    scores = []
    for i in range(out['loc'].shape[0]):
        feat = out['conf_feat'][i]
        p0 = R.openmax_probs(out['conf'][i][:, 1:], feat, mav, fits, rank, dt)
        p1 = R.openmax_probs(out['prop_conf'][i][:, 1:], out['prop_conf_feat'][i] if refined_feature else feat, mav_prop,
                             fits_prop, rank, dt)
        scores.append((((p0 + p1) / dt(2)) * centre_factor(out['center'][i], dt)).T)
    return np.stack(scores)
