"""The OpenMax layer of the ActivityNet1.3 OpenMax baseline on MI355X: common/openmax.py's `OpenMax` and
`compute_eucos_dist` for up to 256 classes (ActivityNet has 150), on the gather kernels of csrc/openmax_wide.hip.

The THUMOS14 kernels stage every class mean vector (MAV) in LDS and end at 16 classes.  openmax_recalibrate
(AFSD/thumos14/openmax.py:42-73) gives a non-zero alpha to the `rank` largest logits only, so a row needs `rank` distances:
the wide kernels gather those MAV rows from memory instead.  Same constructor contract, same buffers, same
results as the narrow layer wherever both apply; there is no CPU fallback.  The Weibull fit, the class means and the
feature view are the shared module's.
"""
import functools

from ..common import openmax as _common
from ..common.openmax import FAMILIES, WeibullFit, class_means, feat_view, weibull_fit_high  # noqa: F401  (re-exported)

MAX_CLASSES, MAX_DIM = FAMILIES['wide'].max_classes, FAMILIES['wide'].max_dim

# openmax.py:7-9 for labelled rows: mav (K, D), feature (N, D) or (B, A, D), int `labels` (N) -> (N,), -1 where the label is
# outside [0, K).  labels None raises NotImplementedError: the all-pairs form is not built at wide K.
compute_eucos_dist = functools.partial(_common.compute_eucos_dist, family='wide')


class OpenMax(_common.OpenMax):
    """thumos14.openmax.OpenMax (openmax.py:12-86) for K <= 256 classes: the same constructor contract (class order, rank
    clamped to K, ValueError for rank < 1, buffers `mav` and `wb`), forward(logits (N, K), feature (N, D)) -> (N, K + 1) float32
    on the device, column 0 = P(unknown), in one launch of otal_openmax_probs_wide.  NotImplementedError beyond K = 256 /
    D = 512."""
    FAMILY = 'wide'
