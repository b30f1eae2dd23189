"""The OpenMax layer of the OpenMax baseline on MI355X, with the reference's names (AFSD/thumos14/openmax.py):
compute_eucos_dist (:7-9) and class OpenMax (:12-86), plus the Weibull tail fit the reference takes from libMR
(experiments/openmax/libMR: MR.fit_high -> MetaRecognition::FitHigh -> EvtGeneric -> weibull_fit; MR.w_score -> CDF ->
weibull_cdf).  The code is common/openmax.py's, shared with the ActivityNet1.3 recipe; this module binds it to the narrow
kernel family (csrc/openmax.hip: K <= 16, every MAV staged in LDS).

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
from ..common.openmax import FAMILIES, TRANSLATE, OpenMax, WeibullFit, class_means, compute_eucos_dist, feat_view, \
    weibull_fit_high  # noqa: F401  (re-exported; OpenMax.FAMILY and compute_eucos_dist's family default to 'narrow')

MAX_CLASSES, MAX_DIM = FAMILIES['narrow'].max_classes, FAMILIES['narrow'].max_dim
