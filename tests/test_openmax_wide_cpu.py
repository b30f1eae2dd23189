"""CPU: the host side of the ActivityNet1.3 OpenMax baseline -- exported symbols and argument errors of
csrc/openmax_wide.hip, the checker's float64 restatement and the float64 Weibull fit against tests/golden/openmax_wide.npz
(tools/pin_openmax_wide.py: the reference's OpenMax over libMR at K = 150), the positives of the statistics pass against
the oracle's ActivityNet matching, and the constructor contract of anet.openmax.OpenMax.  No kernel is launched here."""
import ctypes
import os

import numpy as np
import pytest
import torch

import openmax_ref as R
import openmax_wide_ref as W

K, D, A = W.K, W.D, W.A
SYMBOLS = ("otal_openmax_dist_wide", "otal_openmax_probs_wide", "otal_decode_clips_openmax_wide")


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "openmax_wide.npz"))


@pytest.fixture(scope="module")
def lib():
    from opental_amd.csrc import build
    if not os.path.exists(build.LIB):
        build.build(verbose=False)
    from opental_amd._lib import declare
    return declare(ctypes.CDLL(build.LIB))


def test_wide_symbols_are_exported_and_declared(lib):
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "opental_hip.h")).read()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert f"int {name}(" in header, name
        body = header[:header.index(f"int {name}(")]
        assert body.rstrip().endswith("An additive entry: OTAL_ABI_VERSION is unchanged. */"), name
    assert lib.otal_abi_version() == 26


def test_wide_argument_errors_do_not_launch(lib):
    one = ctypes.c_void_p(16)           # never dereferenced: argument checks come first
    odd = ctypes.c_void_p(20)           # not 16-byte aligned

    def dist(k=150, d=512, mav=one, labels=one, feat=one, out=one, n=4, rpb=4):
        return lib.otal_openmax_dist_wide(feat, n, rpb, 0, d, 1, mav, k, d, labels, out, None)

    def probs(k=150, d=512, r=1, ldl=None, mav=one, logits=one, wb=one, out=one, n=4):
        return lib.otal_openmax_probs_wide(logits, k if ldl is None else ldl, one, n, n, 0, d, 1, mav, wb,
                                           k, d, r, out, None)
    st = (ctypes.c_int64 * 3)(A * 512, 512, 1)

    def decode(c=151, first=1, d=512, r=1, refined=0, mav=one, pmav=one, loc=one, prop_feat=None, pst=None, n=2, flag=one):
        return lib.otal_decode_clips_openmax_wide(loc, one, one, one, one, one, one, one, one, prop_feat, st, pst, mav, pmav, one,
                                                  one, one, one, one, flag, n, A, c, first, d, r, refined, 768.0, 0.001,
                                                  None)
    assert dist(k=257) == -7 and probs(k=257) == -7 and decode(c=258) == -7
    assert dist(k=256, mav=odd) == -7                           # 256 classes are inside the limits: only the alignment refuses
    for bad_d in (528, 504, 8):
        assert dist(d=bad_d) == -7 and probs(d=bad_d) == -7 and decode(d=bad_d) == -7, bad_d
    assert probs(r=0) == -7 and probs(r=151) == -7 and decode(r=0) == -7 and decode(r=151) == -7
    assert probs(k=15, r=16) == -7
    assert dist(mav=odd) == -7 and probs(mav=odd) == -7 and decode(mav=odd) == -7 and decode(pmav=odd) == -7
    assert decode(refined=2, prop_feat=one, pst=st) == -7
    assert dist(labels=None) == -1                              # the all-pairs form is not built
    assert dist(feat=None) == -1 and dist(out=None) == -1
    assert probs(logits=None) == -1 and probs(wb=None) == -1 and probs(out=None) == -1
    assert decode(loc=None) == -1 and decode(flag=None) == -1
    assert decode(refined=1) == -1                              # the refined feature is asked for but not given
    assert probs(ldl=149) == -2                                 # logit rows shorter than K
    assert dist(n=0) == -2 and dist(rpb=0) == -2 and probs(n=0) == -2 and decode(n=0) == -2
    assert decode(c=1) == -2                                    # nothing left once the background logit is dropped
    # the narrow entries keep their limits
    assert lib.otal_openmax_dist(one, 4, 4, 0, 512, 1, one, 17, 512, None, one, None) == -7
    assert lib.otal_openmax_probs(one, 17, one, 4, 4, 0, 512, 1, one, one, 17, 512, 1, one, None) == -7


def test_float64_restatement_equals_the_golden(fx):
    """Pins the checker (tests/openmax_ref.py with k = 150, tests/openmax_wide_ref.py), not the product."""
    cen, pcen = W.mavs(fx)
    for stage, (c, key) in enumerate(((cen, "stat"), (pcen, "prop_stat"))):
        feats, labels = W.stat_rows(c, int(fx["seed_" + key]))
        tails = W.tails_of(W.eucos_own(c[labels], feats), labels)
        assert np.array_equal(tails, fx["fit_tails"][stage * K:(stage + 1) * K])
        assert np.array_equal(tails.min(1), W.fits_of(fx, stage)['small'])
    feats, logits, _ = W.prob_rows(fx)
    for rank in (1, 3):
        p = R.openmax_probs(logits, feats, cen, W.fits_of(fx, 0), rank)
        np.testing.assert_allclose(p, fx[f"probs_r{rank}"], rtol=1e-9, atol=1e-300)
    outs = W.clip_outputs(int(fx["seed_decode"]), cen, pcen)
    args = (cen, W.fits_of(fx, 0), pcen, W.fits_of(fx, 1))
    score = W.decode(outs, *args)
    anchors = fx["decode_anchors"].astype(np.int64)
    assert np.array_equal(anchors, W.DECODE_ANCHORS)
    np.testing.assert_allclose(score[:, :, anchors], fx["decode_score"], rtol=1e-9, atol=1e-300)
    assert np.array_equal(score > fx["decode_params"][0], fx["decode_mask"].astype(bool))
    np.testing.assert_allclose(W.segments(outs, fx["clips"], fx["decode_params"][1]), fx["decode_seg"], rtol=1e-6, atol=1e-6)
    assert np.abs(W.decode(outs, *args, refined_feature=True) - score).max() > 1e-2
    assert np.array_equal(W.priors()[:, 1], np.repeat(np.arange(6), W.LEVELS)) and W.priors().shape == (A, 2)


def test_fixture_keeps_clear_of_the_threshold_and_of_ties(fx):
    """What the pin tool asserted: at most 1 % of the decode cells within 4 * tol_score of conf_thresh; no tied logits."""
    cen, pcen = W.mavs(fx)
    outs = W.clip_outputs(int(fx["seed_decode"]), cen, pcen)
    s = W.decode(outs, cen, W.fits_of(fx, 0), pcen, W.fits_of(fx, 1))[:, 1:]
    near = (np.abs(s - fx["decode_params"][0]) <= 4 * float(fx["tol_score"][0])).sum()
    print(f"{near} of {s.size} cells within 4 * tol_score of the threshold")
    assert near <= 0.01 * s.size
    assert all(len(set(row)) == K for row in W.prob_rows(fx)[1].tolist())


def test_weibull_fit_matches_libmr_on_the_300_tails(fx):
    """weibull_fit_high against libMR's recorded parameters, compared as tests/test_openmax_cpu.py compares them: by the
    w-scores on a grid round each tail (libMR's w_score is the closed formula of its parameters; the pin tool checked that).
    libMR stops its root finder at 1e-6; the pin tool recorded max |w_libMR - w_exact MLE| over these grids as `fit_dev`;
    4x that is allowed -- the factor covers which side of the root libMR lands on."""
    from opental_amd.thumos14.openmax import weibull_fit_high
    bound = 4 * float(fx["fit_dev"])
    assert 0 < bound < 1e-5 and fx["fit_tails"].shape == (2 * K, W.TAILSIZE)
    worst = 0.0
    for tail, (scale, shape, small) in zip(fx["fit_tails"], fx["fit_params"]):
        fit = weibull_fit_high(tail)
        assert fit.small_score == small == tail.min()
        g = W.fit_grid(tail)
        worst = max(worst, float(np.abs(fit.w_score(g) - R.w_score64(g, scale, shape, small)).max()))
    print(f"max |w_fit - w_libMR| = {worst:.3e} (bound {bound:.3e})")
    assert worst <= bound


# ----------------------------------------------------------------------------- the positives of the statistics pass
def oracle_labels(O, monkeypatch, loc, priors, targets, piou):
    """(conf_t, prop_conf_t) of the oracle's ActivityNet matching (oracle.afsd_oracle.multisegment_loss_anet, read-only).  The
    oracle keeps its labels to itself: it hands `logits[pos]` and `labels[pos] - 1` of either stage to its classification
    loss, so that function is replaced by a recorder, and the logits carry the anchor's position in their first column."""
    b, a = loc.shape[:2]
    ids = (torch.arange(b).view(b, 1) * 1000 + torch.arange(a).view(1, a)).float()
    conf = torch.zeros(b, a, 150)
    conf[:, :, 0] = ids
    prop_conf = torch.zeros(b, a, 150)
    prop_conf[:, :, 0] = -ids - 1.0
    got = [torch.zeros(b, a, dtype=torch.long), torch.zeros(b, a, dtype=torch.long)]

    def record(logit, target, *args, **kwargs):
        key = logit[:, 0]
        stage = int(bool((key < 0).all()))
        pos = (-key - 1.0 if stage else key).long()
        got[stage][pos // 1000, pos % 1000] = target.long() + 1
        return logit.sum() * 0.0
    monkeypatch.setattr(O, "evidence_loss_sum_anet", record)
    zeros = torch.zeros(b, a, 1)
    out = dict(loc=loc, conf=conf, prop_loc=torch.zeros(b, a, 2), prop_conf=prop_conf, center=zeros, act=zeros, prop_act=zeros,
               priors=priors)
    O.multisegment_loss_anet(out, targets, piou=piou)
    return got


def test_statistics_pass_positives_equal_the_oracle_matching(monkeypatch):
    from oracle import afsd_oracle as O, arch
    from opental_amd.anet.multisegment_loss import MultiSegmentLoss
    from opental_amd.anet.test_openmax import positive_labels
    cfg = arch.ANET
    pri = O.priors_all(cfg)
    assert np.array_equal(pri.numpy(), W.priors())
    rs = np.random.RandomState(11)
    stride = torch.tensor([cfg["fpn_strides"][int(l)] for l in pri[:, 1]], dtype=torch.float32)
    loc = torch.from_numpy(rs.uniform(0.5, 6.0, (4, A, 2)).astype(np.float32)) * stride.view(1, -1, 1)
    targets = [torch.tensor([[0.10, 0.16, 3.0], [0.30, 0.55, 150.0], [0.60, 0.62, 7.0]]),      # ragged
               torch.tensor([[0.05, 0.95, 41.0]]),                          # 691 frames: only the bounds of levels 4 and 5 admit it
               torch.tensor([[0.5, 0.5 + 2.0 / 768, 7.0]]),                 # 2 frames: inside no level's bounds -> no match
               torch.tensor([[0.20, 0.45, 1.0], [0.25, 0.35, 2.0]])]        # nested: the smaller area wins where both are admitted
    for piou in (0.5, 0.9):
        want_c, want_p = oracle_labels(O, monkeypatch, loc, pri, targets, piou)
        crit = MultiSegmentLoss(151, piou, 1.0, cls_loss_type='focal', os_head=False, clip_length=768)
        conf_t, prop_conf_t = positive_labels(crit, loc, pri, targets)
        assert torch.equal(conf_t, want_c) and torch.equal(prop_conf_t, want_p), piou
        assert int((conf_t[2] > 0).sum()) == 0 and int((prop_conf_t[2] > 0).sum()) == 0
        deep = (conf_t[1] > 0).nonzero().reshape(-1)
        assert len(deep) > 0 and bool((pri[deep, 1] >= 4).all())
        assert 0 < int((prop_conf_t > 0).sum()) < int((conf_t > 0).sum())
        assert set(conf_t[0].unique().tolist()) == {0, 3, 7, 150} and {1, 2} <= set(conf_t[3].unique().tolist())


# ----------------------------------------------------------------------------- the layer's constructor contract
def model_of(fx, k=K, d=D):
    from opental_amd.thumos14.openmax import WeibullFit
    cen = W.mavs(fx)[0]
    scale, shape, small = fx["fit_params"][0]
    return {f"c{i}": {'mean_vec': cen[i % K][:d], 'model': [WeibullFit(scale, shape, small)]} for i in range(k)}


def test_anet_openmax_layer_contract(fx):
    from opental_amd.anet import openmax as AO
    from opental_amd.thumos14 import openmax as TO
    assert AO.weibull_fit_high is TO.weibull_fit_high and AO.class_means is TO.class_means and AO.feat_view is TO.feat_view
    assert AO.WeibullFit is TO.WeibullFit
    model = model_of(fx)
    layer = AO.OpenMax(model, rank=3)
    assert layer.num_cls == K and layer.rank == 3 and layer.class_names == list(model)
    assert layer.mav.shape == (K, D) and layer.wb.shape == (K, 3) and layer.mav.dtype == layer.wb.dtype == torch.float32
    want = np.asarray(TO.WeibullFit(*fx["fit_params"][0]).device_constants(), np.float64).astype(np.float32)
    assert np.array_equal(layer.wb[0].numpy(), want)
    assert AO.OpenMax(model, rank=999).rank == K                # openmax.py:47
    assert AO.OpenMax(model_of(fx, 256)).num_cls == 256
    with pytest.raises(ValueError):
        AO.OpenMax(model, rank=0)
    with pytest.raises(NotImplementedError):
        AO.OpenMax(model_of(fx, 257))
    with pytest.raises(NotImplementedError):
        AO.OpenMax(model_of(fx, 4, 504))
    with pytest.raises(RuntimeError):                           # host tensors: there is no CPU fallback
        layer(torch.zeros(4, K), torch.zeros(4, D))
    with pytest.raises(RuntimeError):
        AO.compute_eucos_dist(torch.zeros(K, D), torch.zeros(4, D), torch.zeros(4, dtype=torch.int32))
    with pytest.raises(NotImplementedError):                    # the narrow layer keeps its limit
        TO.OpenMax(model_of(fx, 17))
    # one statistics pass, one set of file helpers and one decode wrapper serve both recipes
    from opental_amd.anet import test_openmax as ATO
    from opental_amd.common import openmax as CO
    from opental_amd.thumos14 import test_openmax as TTO
    for mod, family in ((TTO, 'narrow'), (ATO, 'wide')):
        assert mod.mav_and_dist.func is CO.mav_and_dist and mod.mav_and_dist.keywords == {'family': family}
        assert mod.save_mav_dist is CO.save_mav_dist and mod.weibull_fitting is CO.weibull_fitting
        assert mod.files_are_ready is CO.files_are_ready
    assert TTO.decode_clips_openmax is CO.decode_clips_openmax
    assert AO.compute_eucos_dist.func is TO.compute_eucos_dist is CO.compute_eucos_dist
    # a narrow and a wide layer of equal K do not decode together: refused first (their ranks differ too), on host tensors
    narrow, wide = TO.OpenMax(model_of(fx, 15), rank=1), AO.OpenMax(model_of(fx, 15), rank=3)
    z = lambda *shape: torch.zeros(shape)
    host = dict(loc=z(2, A, 2), prop_loc=z(2, A, 2), conf=z(2, A, 16), prop_conf=z(2, A, 16), center=z(2, A, 1),
                conf_feat=z(2, A, D), prop_conf_feat=z(2, A, D), priors=z(A, 2))
    with pytest.raises(RuntimeError, match="one kernel family"):
        CO.decode_clips_openmax(host, [0.0, 0.0], 30.0, narrow, wide, 768, 0.001)
    with pytest.raises(RuntimeError, match="one kernel family"):                # the recipe's wrapper goes through it
        ATO.decode_clips_openmax(host, 30.0, wide, narrow)
    with pytest.raises(RuntimeError, match="same rank"):
        CO.decode_clips_openmax(host, [0.0, 0.0], 30.0, wide, AO.OpenMax(model_of(fx, 15), rank=1), 768, 0.001)


def test_driver_module_imports_without_a_device():
    """... and its docstring, which defines the behaviour, names the command line."""
    from opental_amd.anet import test_openmax as ATO
    assert "python -m opental_amd.anet.test_openmax" in ATO.__doc__ and ATO.TAILSIZE == 20
