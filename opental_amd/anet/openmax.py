"""The OpenMax layer of the ActivityNet1.3 OpenMax baseline on MI355X: thumos14/openmax.py's `OpenMax` and
`compute_eucos_dist` for up to 256 classes (ActivityNet has 150), on the gather kernels of csrc/openmax_wide.hip.

The THUMOS14 kernels stage every class mean vector (MAV) in LDS and end at 16 classes.  openmax_recalibrate
(AFSD/thumos14/openmax.py:42-73) gives a non-zero alpha to the `rank` largest logits only, so a row needs `rank` distances:
the wide kernels gather those MAV rows from memory instead.  Same constructor contract, same buffers, same
results as the narrow layer wherever both apply; there is no CPU fallback.  The Weibull fit, the class means and the
feature view are the THUMOS14 module's.
"""
import ctypes

import torch

from .. import _lib as L
from ..thumos14 import openmax as _narrow
from ..thumos14.openmax import WeibullFit, class_means, feat_view, weibull_fit_high  # noqa: F401  (re-exported)

MAX_CLASSES, MAX_DIM = 256, 512        # csrc/openmax_wide.hip: 16 class slots on each of 16 lanes; the staged feature row


def _i64(v):
    return ctypes.c_int64(int(v))


def compute_eucos_dist(mav, feature, labels):
    """openmax.py:7-9 for labelled rows: ||mav - f||_2 / 200 + (1 - cos(mav, f)) of row n against mav[labels[n]].  mav (K, D),
    feature (N, D) or (B, A, D), possibly a strided view, int `labels` (N) -> (N,), -1 where the label is outside [0, K).
    (The all-pairs (N, K) form of the THUMOS14 module is not built at wide K: nothing uses it.)"""
    if labels is None:
        raise NotImplementedError("anet.openmax.compute_eucos_dist computes labelled distances only")
    mav = mav.to(torch.float32).contiguous()
    K, D = mav.shape
    rpb, sb, sr, sc = feat_view(feature)
    N = feature.numel() // feature.shape[-1]
    if feature.shape[-1] != D:
        raise RuntimeError(f"feature dimension {feature.shape[-1]} != MAV dimension {D}")
    labels = labels.to(torch.int32).contiguous()
    if labels.numel() != N:
        raise RuntimeError("one label per feature row")
    out = torch.empty((N,), dtype=torch.float32, device=feature.device)
    L.check(L.lib().otal_openmax_dist_wide(L.ptr(feature), N, rpb, _i64(sb), _i64(sr), _i64(sc), L.ptr(mav), K, D,
                                           L.ptr(labels), L.ptr(out), L.stream()), "otal_openmax_dist_wide")
    return out


class OpenMax(_narrow.OpenMax):
    """thumos14.openmax.OpenMax (openmax.py:12-86) for K <= 256 classes: the same constructor contract (class order, rank
    clamped to K, ValueError for rank < 1, buffers `mav` and `wb`), forward(logits (N, K), feature (N, D)) -> (N, K + 1) float32
    on the device, column 0 = P(unknown), in one launch of otal_openmax_probs_wide.  NotImplementedError beyond K = 256 /
    D = 512."""
    MAX_CLASSES, MAX_DIM = MAX_CLASSES, MAX_DIM
    ENTRY = "otal_openmax_probs_wide"
