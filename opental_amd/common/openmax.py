"""What the OpenMax baselines of both recipes (thumos14/, anet/) share, written once: the OpenMax layer, the eucos distance,
the class means, the Weibull tail fit (thumos14/openmax.py's docstring states the fit), the batched decode wrapper, the
statistics of the positive anchors and the mav_dist files.

Two kernel families serve them (FAMILIES): `narrow` (csrc/openmax.hip, K <= 16, every MAV staged in LDS; THUMOS14) and
`wide` (csrc/openmax_wide.hip, K <= 256, MAV rows gathered; ActivityNet1.3).  They order their sums differently and give
different bits.  A layer's family is its class attribute FAMILY; the decode wrapper takes its entry from the layers, the
distance from its `family` argument.  There is no CPU fallback.
"""
import collections
import ctypes
import math
import os

import numpy as np
import torch
import torch.nn as nn

from .. import _lib as L
from .detect import clip_scalars

TRANSLATE = 10000.0

# a kernel family: what one workgroup handles and the entry points (same arguments in both families)
Family = collections.namedtuple('Family', 'max_classes max_dim dist probs decode')
FAMILIES = {
    'narrow': Family(16, 512, "otal_openmax_dist", "otal_openmax_probs", "otal_decode_clips_openmax"),
    'wide': Family(256, 512, "otal_openmax_dist_wide", "otal_openmax_probs_wide", "otal_decode_clips_openmax_wide"),
}


def feat_view(feature):
    """(rows_per_batch, sb, sr, sc) element strides of a (N, D) or (B, A, D) float32 device tensor, read in place."""
    if feature.dtype != torch.float32 or not feature.is_cuda:
        raise RuntimeError("OpenMax runs on float32 device tensors only (there is no CPU fallback)")
    if feature.dim() == 2:
        return feature.shape[0], 0, feature.stride(0), feature.stride(1)
    if feature.dim() == 3:
        return feature.shape[1], feature.stride(0), feature.stride(1), feature.stride(2)
    raise RuntimeError(f"feature must be (N, D) or (B, A, D), got {tuple(feature.shape)}")


def compute_eucos_dist(mav, feature, labels=None, family='narrow'):
    """openmax.py:7-9 for many rows: ||mav - f||_2 / 200 + (1 - cos(mav, f)).  mav (K, D) or (D,), feature (N, D) or (B, A, D),
    possibly a strided view; -> (N, K) (all rows against all MAVs), or with int32 `labels` (N) -> (N,), row n against
    mav[labels[n]] (-1 where the label is outside [0, K)).  The all-pairs form is not built at wide K: nothing uses it."""
    entry = FAMILIES[family].dist
    if labels is None and family == 'wide':
        raise NotImplementedError(f"{entry} computes labelled distances only")
    mav = mav.reshape(1, -1) if mav.dim() == 1 else mav
    mav = mav.to(torch.float32).contiguous()
    K, D = mav.shape
    rpb, sb, sr, sc = feat_view(feature)
    N = feature.numel() // feature.shape[-1]
    if feature.shape[-1] != D:
        raise RuntimeError(f"feature dimension {feature.shape[-1]} != MAV dimension {D}")
    out = torch.empty((N,) if labels is not None else (N, K), dtype=torch.float32, device=feature.device)
    if labels is not None:
        labels = labels.to(torch.int32).contiguous()
        if labels.numel() != N:
            raise RuntimeError("one label per feature row")
    L.check(getattr(L.lib(), entry)(L.ptr(feature), N, rpb, sb, sr, sc, L.ptr(mav), K, D,
                                    None if labels is None else L.ptr(labels), L.ptr(out), L.stream()), entry)
    return out


def class_means(feature, labels, num_classes):
    """Per-class mean of labelled feature rows (test_openmax.py:317-318): (K, D) means and (K,) int32 counts; labels outside
    [0, K) are ignored.  Fixed summation order: two runs give the same bits."""
    rpb, sb, sr, sc = feat_view(feature)
    D = feature.shape[-1]
    N = feature.numel() // D
    labels = labels.to(torch.int32).contiguous()
    if labels.numel() != N:
        raise RuntimeError("one label per feature row")
    means = torch.empty((num_classes, D), dtype=torch.float32, device=feature.device)
    counts = torch.empty((num_classes,), dtype=torch.int32, device=feature.device)
    L.check(L.lib().otal_openmax_class_means(L.ptr(feature), N, rpb, sb, sr, sc, L.ptr(labels),
                                             num_classes, D, L.ptr(means), L.ptr(counts), L.stream()),
            "otal_openmax_class_means")
    return means, counts


class WeibullFit:
    """What libMR's MR object holds after fit_high: Weibull (scale, shape) of the translated tail, the tail's smallest
    value and the translation.  w_score is float64, libMR's formula (MetaRecognition.cpp:141-152, weibull.c:79-104)."""

    def __init__(self, scale, shape, small_score, translate=TRANSLATE):
        self.scale, self.shape, self.small_score, self.translate = float(scale), float(shape), float(small_score), float(translate)

    def w_score(self, d):
        x = np.asarray(d, np.float64) + self.translate - self.small_score
        with np.errstate(invalid='ignore'):
            w = np.where(x < 0, 0.0, 1.0 - np.exp(-np.power(np.maximum(x, 0.0) / self.scale, self.shape)))
        return float(w) if np.ndim(d) == 0 else w

    def device_constants(self):
        """(off, 1 / scale, shape) for the kernel's fp32 form: w = -expm1(-exp(shape * log1p((d - off) / scale))); the
        translated argument over scale is 1 + (d - off) / scale with off = small + (scale - translate), formed in float64."""
        return (self.small_score + (self.scale - self.translate), 1.0 / self.scale, self.shape)


def _likelihood(sigma, y0, ybar):
    e = np.exp(y0 / sigma)
    return sigma + ybar - float(np.sum(y0 * e) / np.sum(e))


def weibull_fit_high(tail, name=None, translate=TRANSLATE):
    """libMR's MR().fit_high(tail, len(tail)) in float64 (see the module docstring) -> WeibullFit."""
    who = "" if name is None else f" of class {name!r}"
    d = np.sort(np.asarray([float(v) for v in tail], np.float64))[::-1]
    if d.size < 2 or not np.all(np.isfinite(d)):
        raise ValueError(f"Weibull fit{who}: the tail needs at least two finite distances, got {d.size}")
    small = float(d[-1])
    x = d + translate - small
    if np.any(x <= 0):
        raise ValueError(f"Weibull fit{who}: non-positive translated value")
    y = np.log(x)
    ymax, rng = float(y.max()), float(y.max() - y.min())
    if not rng > 0:
        raise ValueError(f"Weibull fit{who}: the tail has fewer than two distinct values")
    y0 = (y - ymax) / rng
    n = y0.size
    ybar = float(np.sum(y0) / n)
    sigma0 = math.sqrt(6.0) * float(np.sqrt(np.sum((y0 - ybar) ** 2) / (n - 1))) / math.pi
    if _likelihood(sigma0, y0, ybar) > 0:
        upper, lower = sigma0, 0.5 * sigma0
        while _likelihood(lower, y0, ybar) > 0:
            upper, lower = lower, 0.5 * lower
            if lower < 1e-300:
                raise ValueError(f"Weibull fit{who}: the likelihood equation has no root (underflow)")
    else:
        lower, upper = sigma0, 2.0 * sigma0
        while _likelihood(upper, y0, ybar) < 0:
            lower, upper = upper, 2.0 * upper
            if upper > 1e300:
                raise ValueError(f"Weibull fit{who}: the likelihood equation has no root (overflow)")
    for _ in range(200):                    # g(lower) <= 0 <= g(upper): bisect until the bracket is one ulp wide
        mid = 0.5 * (lower + upper)
        if mid <= lower or mid >= upper:
            break
        if _likelihood(mid, y0, ybar) > 0:
            upper = mid
        else:
            lower = mid
    sigma = 0.5 * (lower + upper)
    mu = sigma * math.log(float(np.sum(np.exp(y0 / sigma))) / n)
    return WeibullFit(math.exp(rng * mu + ymax), 1.0 / (rng * sigma), small, translate)


class OpenMax(nn.Module):
    """openmax.py:12-86.  weibull_model: {class name: {'mean_vec': (D,), 'model': [fit]}} in class order, fit = WeibullFit (or
    any object with scale / shape / small_score / translate).  forward(logits (N, K), feature (N, D)) -> (N, K + 1) float32 on
    the device, column 0 = P(unknown), in one launch.  rank: how many top logits are recalibrated (1 <= rank <= K; equal
    logits rank the higher index first, as numpy's argsort()[::-1] does)."""
    FAMILY = 'narrow'           # the key of FAMILIES; anet.openmax.OpenMax has 'wide'

    def __init__(self, weibull_model, rank=1):
        super().__init__()
        fam = FAMILIES[self.FAMILY]
        self.weibull_model = weibull_model
        self.class_names = list(weibull_model.keys())
        self.num_cls = len(self.class_names)
        self.rank = min(self.num_cls, int(rank))            # openmax.py:47
        if not 1 <= self.rank:
            raise ValueError("rank must be at least 1")
        mav = np.stack([np.asarray(weibull_model[n]['mean_vec'], np.float32).reshape(-1) for n in self.class_names], 0)
        wb = np.array([_constants(weibull_model[n]['model'][0]) for n in self.class_names], np.float64)
        if self.num_cls > fam.max_classes or mav.shape[1] > fam.max_dim or mav.shape[1] % 16:
            raise NotImplementedError(f"OpenMax kernel ({fam.probs}): K <= {fam.max_classes}, D <= {fam.max_dim}, D % 16 == 0; "
                                      f"got K = {self.num_cls}, D = {mav.shape[1]}")
        self.register_buffer('mav', torch.from_numpy(mav), persistent=False)
        self.register_buffer('wb', torch.from_numpy(wb.astype(np.float32)), persistent=False)

    def tensors(self, device):
        if self.mav.device != device:
            self.to(device)
        return self.mav, self.wb

    def forward(self, logits_in, feature_in):
        K = self.num_cls
        if logits_in.dim() != 2 or logits_in.shape[1] != K or feature_in.dim() != 2 or feature_in.shape[0] != logits_in.shape[0]:
            raise RuntimeError(f"OpenMax.forward: logits (N, {K}) and feature (N, D) expected")
        logits = logits_in if (logits_in.dtype == torch.float32 and logits_in.stride(1) == 1) else logits_in.float().contiguous()
        rpb, sb, sr, sc = feat_view(feature_in)
        mav, wb = self.tensors(feature_in.device)
        N, D = feature_in.shape
        if D != mav.shape[1]:
            raise RuntimeError(f"feature dimension {D} != MAV dimension {mav.shape[1]}")
        out = torch.empty((N, K + 1), dtype=torch.float32, device=feature_in.device)
        entry = FAMILIES[self.FAMILY].probs
        L.check(getattr(L.lib(), entry)(L.ptr(logits), logits.stride(0), L.ptr(feature_in), N, rpb, sb, sr,
                                        sc, L.ptr(mav), L.ptr(wb), K, D, self.rank, L.ptr(out), L.stream()), entry)
        return out


def _constants(fit):
    if hasattr(fit, 'device_constants'):
        return fit.device_constants()
    return WeibullFit(fit.scale, fit.shape, fit.small_score, getattr(fit, 'translate', TRANSLATE)).device_constants()


def decode_clips_openmax(output_dict, offsets, fps, openmax_layer, openmax_prop_layer, clip_length=256, conf_thresh=0.01,
                         refined_feature=False):
    """Batched decode_output (test_openmax.py:141-170) + the threshold test of `filtering` (:173-174) in one launch of the
    layers' family: both stages' recalibration, their average, the centre factor, the segments and flag = score >
    conf_thresh (the defaults are the reference's, THUMOS14's).  output_dict: the closed-set network's outputs for n clips
    with get_feat=True (conf / prop_conf carry the background logit, which is dropped; priors (A) centres).  Returns
    dict(seg (n, A, 2), score (n, K, A), flag (n, K, A) uint8, unknown (n, A), unct None, actn None): the layout of
    decode_clips, so softnms_classes takes it as it is (3-column rows).  Every check precedes the first device pointer."""
    if openmax_layer.FAMILY != openmax_prop_layer.FAMILY:
        raise RuntimeError(f"the two OpenMax layers must be of one kernel family, got {openmax_layer.FAMILY} and "
                           f"{openmax_prop_layer.FAMILY}")
    entry = FAMILIES[openmax_layer.FAMILY].decode
    loc = output_dict['loc'].contiguous()
    n, A, _ = loc.shape
    C = output_dict['conf'].shape[-1]
    K = openmax_layer.num_cls
    if C != K + 1 or openmax_prop_layer.num_cls != K:
        raise RuntimeError(f"OpenMax decode: {C} logits per anchor for {K} Weibull models (a closed-set head has K + 1)")
    if openmax_layer.rank != openmax_prop_layer.rank:
        raise RuntimeError("the two OpenMax layers must use the same rank")
    dev = loc.device
    feat, prop_feat = output_dict['conf_feat'], output_dict['prop_conf_feat'] if refined_feature else None
    D = feat.shape[-1]
    strides = lambda t: (ctypes.c_int64 * 3)(*t.stride())
    for t in (feat, prop_feat):
        if t is not None and (t.dtype != torch.float32 or not t.is_cuda or tuple(t.shape) != (n, A, D)):
            raise RuntimeError("conf_feat / prop_conf_feat must be (n, A, D) float32 device tensors")
    offs, fpst = clip_scalars(offsets, fps, n, dev)
    mav, wb = openmax_layer.tensors(dev)
    pmav, pwb = openmax_prop_layer.tensors(dev)
    seg = torch.empty((n, A, 2), device=dev)
    score = torch.empty((n, K, A), device=dev)
    unknown = torch.empty((n, A), device=dev)
    flag = torch.empty((n, K, A), dtype=torch.uint8, device=dev)
    t = lambda k: output_dict[k].contiguous()
    L.check(getattr(L.lib(), entry)(
        L.ptr(loc), L.ptr(t('prop_loc')), L.ptr(t('priors')), L.ptr(t('conf')), L.ptr(t('prop_conf')), L.ptr(t('center')),
        L.ptr(offs), L.ptr(fpst), L.ptr(feat), None if prop_feat is None else L.ptr(prop_feat), strides(feat),
        None if prop_feat is None else strides(prop_feat), L.ptr(mav), L.ptr(pmav), L.ptr(wb), L.ptr(pwb), L.ptr(seg),
        L.ptr(score), L.ptr(unknown), L.ptr(flag), n, A, C, 1, D, openmax_layer.rank, 1 if refined_feature else 0,
        clip_length, conf_thresh, L.stream()), entry)
    return dict(seg=seg, score=score, unct=None, actn=None, flag=flag, unknown=unknown)


def positive_rows(out, conf_t, prop_conf_t):
    """The tower features (rows of out['conf_feat'] / out['prop_conf_feat']) and 0-based int32 class indices of the positive
    anchors of both stages: conf_t > 0 selects the coarse rows, prop_conf_t > 0 the refined ones (test_openmax.py:290-311).
    -> (feat (P, D), labels (P,), prop_feat, prop_labels) of this batch."""
    rows = []
    for ft, lab in ((out['conf_feat'], conf_t), (out['prop_conf_feat'], prop_conf_t)):
        pos = lab.reshape(-1) > 0
        rows += [ft.reshape(-1, ft.shape[-1])[pos], (lab.reshape(-1)[pos] - 1).to(torch.int32)]
    return tuple(rows)


def cat_rows(batches):
    """positive_rows of every batch of a statistics pass -> the four contiguous tensors of the pass."""
    return tuple(torch.cat(xs, 0).contiguous() for xs in zip(*batches))


def mav_and_dist(feat, labels, num_classes, family):
    """Per class: MAV = float32 mean of its rows, dist = eucos distance of each of its rows to that MAV
    (test_openmax.py:316-324), with the class-means kernel and the family's labelled distance kernel.  -> mav (K, D),
    counts (K,), dist (N,) on the device."""
    if feat.shape[0] == 0:
        return (torch.zeros((num_classes, feat.shape[1]), device=feat.device),
                torch.zeros((num_classes,), dtype=torch.int32, device=feat.device), torch.zeros((0,), device=feat.device))
    mav, counts = class_means(feat, labels, num_classes)
    return mav, counts, compute_eucos_dist(mav, feat, labels, family)


def save_mav_dist(mav_dist_dir, idx_to_class, stats, prop_stats):
    """One <class name>.npz per class with the reference's keys (test_openmax.py:326-327).  stats = (mav, counts, dist,
    labels) of the coarse stage, prop_stats of the refined one.  A class without a positive anchor raises (the reference
    fails in np.stack([]))."""
    os.makedirs(mav_dist_dir, exist_ok=True)
    host = [[np.asarray(t.cpu().numpy()) for t in s] for s in (stats, prop_stats)]
    names = [idx_to_class[c] for c in sorted(idx_to_class)]
    for stage, (_, counts, _, _) in zip(("coarse", "refined"), host):
        empty = [n for k, n in enumerate(names) if counts[k] == 0]
        if empty:
            raise ValueError(f"compute_mav_dist: no positive {stage}-stage anchor for class(es) {', '.join(empty)}: "
                             "the training split must hold every known class (and, for the refined stage, proposals "
                             "whose tIoU reaches training.piou)")
    for k, name in enumerate(names):
        (mav, _, dist, lab), (pmav, _, pdist, plab) = host
        np.savez(os.path.join(mav_dist_dir, f'{name}.npz'), mav=mav[k], dist=dist[lab == k], mav_prop=pmav[k],
                 dist_prop=pdist[plab == k])


def files_are_ready(mav_dist_dir, idx_to_class):
    """test_openmax.py:407-414."""
    return all(os.path.exists(os.path.join(mav_dist_dir, f'{n}.npz')) for n in idx_to_class.values())


def weibull_fitting(idx_to_class, mav_dist_dir, tailsize=20):
    """test_openmax.py:331-354: per class and stage the `tailsize` largest distances -> weibull_fit_high.  Returns the
    reference's two dicts {name: {'mean_vec', 'model': [fit]}}."""
    weibull_model, weibull_prop_model = {}, {}
    for cl in sorted(idx_to_class):
        name = idx_to_class[cl]
        data = np.load(os.path.join(mav_dist_dir, f'{name}.npz'), allow_pickle=True)
        for model, mav, dist in ((weibull_model, data['mav'], data['dist']), (weibull_prop_model, data['mav_prop'], data['dist_prop'])):
            tail = sorted(dist)[-tailsize:]
            model[name] = {'mean_vec': mav, 'model': [weibull_fit_high(tail, name)]}
    return weibull_model, weibull_prop_model
