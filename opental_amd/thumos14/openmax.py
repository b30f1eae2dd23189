"""The OpenMax layer of the OpenMax baseline on MI355X, with the reference's names (AFSD/thumos14/openmax.py):
compute_eucos_dist (:7-9) and class OpenMax (:12-86), plus the Weibull tail fit the reference takes from libMR
(experiments/openmax/libMR: MR.fit_high -> MetaRecognition::FitHigh -> EvtGeneric -> weibull_fit; MR.w_score -> CDF ->
weibull_cdf).

The reference's forward copies logits and features to the host and loops in Python over every row and class with two scipy
calls and a libMR call each; here `OpenMax.forward` is ONE launch (otal_openmax_probs, csrc/openmax.hip) on device tensors.
There is no CPU fallback.

`weibull_fit_high` is this project's own float64 statement of the fit, written from the equations:
  tail d_1..d_n (the n largest distances), small = min d, x_i = d_i + translate - small (translate = 10000);
  y_i = log x_i follows a smallest-extreme-value law with location mu and scale sigma; with the y_i shifted and scaled to
  y0_i = (y_i - max y) / (max y - min y) in [-1, 0] the likelihood equation for sigma is
      g(sigma) = sigma + mean(y0) - sum(y0 * exp(y0 / sigma)) / sum(exp(y0 / sigma)) = 0,
  mu = sigma * log(mean(exp(y0 / sigma))); back in the original units Weibull scale = exp(range * mu + max y) and
  shape = 1 / (range * sigma).
The root is bracketed as libMR does -- from sqrt(6) * std(y0) / pi, halving or doubling until g changes sign -- and then
bisected to the last bit (libMR stops at 1e-6, so its parameters differ from the exact MLE by its own stopping error).
Deviation from libMR: a degenerate tail (fewer than two distinct values, a non-positive translated value) raises ValueError
naming the class; libMR leaves the object invalid and silently returns -9999 as every w-score.
"""
import ctypes
import math

import numpy as np
import torch
import torch.nn as nn

from .. import _lib as L

TRANSLATE = 10000.0
MAX_CLASSES, MAX_DIM = 16, 512         # what one workgroup of csrc/openmax.hip stages


def feat_view(feature):
    """(rows_per_batch, sb, sr, sc) element strides of a (N, D) or (B, A, D) float32 device tensor, read in place."""
    if feature.dtype != torch.float32 or not feature.is_cuda:
        raise RuntimeError("OpenMax runs on float32 device tensors only (there is no CPU fallback)")
    if feature.dim() == 2:
        return feature.shape[0], 0, feature.stride(0), feature.stride(1)
    if feature.dim() == 3:
        return feature.shape[1], feature.stride(0), feature.stride(1), feature.stride(2)
    raise RuntimeError(f"feature must be (N, D) or (B, A, D), got {tuple(feature.shape)}")


def _i64(v):
    return ctypes.c_int64(int(v))


def compute_eucos_dist(mav, feature, labels=None):
    """openmax.py:7-9 for many rows: ||mav - f||_2 / 200 + (1 - cos(mav, f)).  mav (K, D) or (D,), feature (N, D) or (B, A, D),
    possibly a strided view; -> (N, K) (all rows against all MAVs), or with int32 `labels` (N) -> (N,), row n against
    mav[labels[n]] (-1 where the label is outside [0, K))."""
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
    L.check(L.lib().otal_openmax_dist(L.ptr(feature), N, rpb, _i64(sb), _i64(sr), _i64(sc), L.ptr(mav), K, D,
                                      None if labels is None else L.ptr(labels), L.ptr(out), L.stream()), "otal_openmax_dist")
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
    L.check(L.lib().otal_openmax_class_means(L.ptr(feature), N, rpb, _i64(sb), _i64(sr), _i64(sc), L.ptr(labels),
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
    # the kernel's limits and its entry point; anet.openmax.OpenMax overrides them with the wide kernel's (same arguments)
    MAX_CLASSES, MAX_DIM, ENTRY = MAX_CLASSES, MAX_DIM, "otal_openmax_probs"

    def __init__(self, weibull_model, rank=1):
        super().__init__()
        self.weibull_model = weibull_model
        self.class_names = list(weibull_model.keys())
        self.num_cls = len(self.class_names)
        self.rank = min(self.num_cls, int(rank))            # openmax.py:47
        if not 1 <= self.rank:
            raise ValueError("rank must be at least 1")
        mav = np.stack([np.asarray(weibull_model[n]['mean_vec'], np.float32).reshape(-1) for n in self.class_names], 0)
        wb = np.array([_constants(weibull_model[n]['model'][0]) for n in self.class_names], np.float64)
        if self.num_cls > self.MAX_CLASSES or mav.shape[1] > self.MAX_DIM or mav.shape[1] % 16:
            raise NotImplementedError(f"OpenMax kernel ({self.ENTRY}): K <= {self.MAX_CLASSES}, D <= {self.MAX_DIM}, D % 16 == 0; "
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
        L.check(getattr(L.lib(), self.ENTRY)(L.ptr(logits), _i64(logits.stride(0)), L.ptr(feature_in), N, rpb, _i64(sb), _i64(sr),
                                             _i64(sc), L.ptr(mav), L.ptr(wb), K, D, self.rank, L.ptr(out), L.stream()),
                self.ENTRY)
        return out


def _constants(fit):
    if hasattr(fit, 'device_constants'):
        return fit.device_constants()
    return WeibullFit(fit.scale, fit.shape, fit.small_score, getattr(fit, 'translate', TRANSLATE)).device_constants()
