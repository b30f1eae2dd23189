"""float64 numpy restatement of the RPL / GCPL baselines' distance head, its backward and the two classification terms of
the detection loss -- the independent reference of tests/test_rpl_cpu.py and tests/test_rpl_gpu.py (the role
tests/openmax_ref.py plays for OpenMax).  Written from the formulas, not from the package:

    dist[b, c, n]   = mean_d (x[b, d, n] - centers[c, d])^2
    dx[b, d, n]     = 2/D sum_c g[b, c, n] (x[b, d, n] - centers[c, d])
    dcenters[c, d]  = 2/D sum_{b, n} g[b, c, n] (centers[c, d] - x[b, d, n])

and, with A anchors, CE_i the softmax cross-entropy of row i against label y_i, d_i = dist[i, y_i]:

    RPL   coarse (sum CE(dist / T) + w sum (d - r)^2) / N       refined ((1/A) sum CE(dist / T) + (w/A) sum (d - r)^2) / PN
    GCPL  coarse (sum CE(-dist / T) + w/(2A) sum d) / N         refined ((1/A) sum CE(-dist / T) + w/(2A) sum d) / PN
"""
import numpy as np

FEAT_SEED, CENTER_SEED, GRAD_SEED = 515, 616, 717      # tools/pin_rpl.py draws from the same seeds
B, D, N, C = 2, 512, 126, 16


def seeded_inputs(b=B, c=C, d=D, n=N):
    """(coarse features, refined features, coarse centres, refined centres, upstream gradient of the head) in float32:
    relu(randn) features, 0.1 * randn centres, randn gradient -- what tools/pin_rpl.py fed the reference."""
    rs = np.random.RandomState(FEAT_SEED)
    feats = [np.maximum(rs.standard_normal((b, d, n)), 0.0).astype(np.float32) for _ in range(2)]
    rs = np.random.RandomState(CENTER_SEED)
    cens = [(0.1 * rs.standard_normal((c, d))).astype(np.float32) for _ in range(2)]
    g = np.random.RandomState(GRAD_SEED).standard_normal((b, c, n)).astype(np.float32)
    return feats[0], feats[1], cens[0], cens[1], g


def head_fwd(x, centers):
    x, centers = np.asarray(x, np.float64), np.asarray(centers, np.float64)
    diff = x[:, None, :, :] - centers[None, :, :, None]               # (B, C, D, N)
    return (diff * diff).mean(2)


def head_bwd(x, centers, g):
    x, centers, g = np.asarray(x, np.float64), np.asarray(centers, np.float64), np.asarray(g, np.float64)
    Dn = x.shape[1]
    gs = g.sum(1)                                                       # (B, N)
    dx = 2.0 / Dn * (x * gs[:, None, :] - np.einsum('bcn,cd->bdn', g, centers))
    dcen = 2.0 / Dn * (centers * g.sum((0, 2))[:, None] - np.einsum('bcn,bdn->cd', g, x))
    return dx, dcen


def match(loc, priors, targets, clip=256.0, overlap=0.5):
    """Anchor <-> ground-truth assignment (labels of the coarse and of the refined stage), per sample."""
    loc = np.asarray(loc, np.float64)
    conf_t = np.zeros(loc.shape[:2], np.int64)
    prop_t = np.zeros(loc.shape[:2], np.int64)
    p = np.asarray(priors, np.float64).reshape(-1)
    for b, t in enumerate(targets):
        t = np.asarray(t, np.float64)
        left = (p[:, None] - t[None, :, 0]) * clip
        right = (t[None, :, 1] - p[:, None]) * clip
        area = left + right
        area[(left < 0) | (right < 0)] = 2 * clip
        best = area.argmin(1)
        lab = t[best, 2].astype(np.int64)
        lab[area.min(1) >= 2 * clip] = 0
        lt = np.stack([(p - t[best, 0]) * clip, (t[best, 1] - p) * clip], -1)
        inter = np.minimum(loc[b, :, 0], lt[:, 0]) + np.minimum(loc[b, :, 1], lt[:, 1])
        union = lt.sum(1) + loc[b].sum(1) - inter
        iou = inter / np.maximum(union, np.finfo(np.float32).eps)
        conf_t[b] = lab
        prop_t[b] = np.where(iou < overlap, 0, lab)
    return conf_t, prop_t


def cls_term(dist, labels, norm, refined, gcpl, temperature=1.0, weight_pl=0.1, radius=0.0):
    """One classification term and its gradient with respect to dist (A, C); labels (A,)."""
    dist = np.asarray(dist, np.float64)
    A = dist.shape[0]
    sgn = -1.0 if gcpl else 1.0
    z = sgn * dist / temperature
    z = z - z.max(1, keepdims=True)
    lse = np.log(np.exp(z).sum(1))
    p = np.exp(z - lse[:, None])
    rows = np.arange(A)
    ce = lse - z[rows, labels]
    onehot = np.zeros_like(dist)
    onehot[rows, labels] = 1.0
    ce_w = 1.0 / A if refined else 1.0
    d = dist[rows, labels]
    if gcpl:
        reg, dreg = weight_pl / (2 * A) * d.sum(), np.full(A, weight_pl / (2 * A))
    else:
        rw = weight_pl / A if refined else weight_pl
        reg, dreg = rw * ((d - radius) ** 2).sum(), rw * 2 * (d - radius)
    term = (ce_w * ce.sum() + reg) / norm
    grad = (ce_w * sgn / temperature * (p - onehot) + onehot * dreg[:, None]) / norm
    return term, grad


def cls_terms_and_grads(feats_c, feats_p, cen_c, cen_p, loc, priors, targets, gcpl, overlap=0.5, **kw):
    """(loss_c, loss_prop_c) and their gradients (not yet weighted) with respect to the two feature maps and centre tables."""
    conf_t, prop_t = match(loc, priors, targets, overlap=overlap)
    Nn, PN = max(int((conf_t > 0).sum()), 1), max(int((prop_t > 0).sum()), 1)
    out = []
    for x, cen, lab, norm, refined in ((feats_c, cen_c, conf_t, Nn, False), (feats_p, cen_p, prop_t, PN, True)):
        dist = head_fwd(x, cen)                                         # (B, C, N)
        Bn, Cn, Nk = dist.shape
        rows = dist.transpose(0, 2, 1).reshape(-1, Cn)
        term, g = cls_term(rows, lab.reshape(-1), norm, refined, gcpl, **kw)
        dx, dcen = head_bwd(x, cen, g.reshape(Bn, Nk, Cn).transpose(0, 2, 1))
        out.append((term, dx, dcen))
    return out
