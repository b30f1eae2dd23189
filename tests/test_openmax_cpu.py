"""CPU: the OpenMax baseline's host side -- exported symbols and argument errors of csrc/openmax.hip, the float64 Weibull
fit against libMR (tests/golden/openmax.npz, tools/pin_openmax.py), the checker's own float64 restatement against the golden,
the mav_dist files and the matching plumbing.  No kernel is launched here."""
import ctypes
import os

import numpy as np
import pytest
import torch

import openmax_ref as R

K, D, A = R.K, R.D, R.A
NAMES = [f"class_{i}" for i in range(1, K + 1)]
SYMBOLS = ("otal_openmax_dist", "otal_openmax_class_means", "otal_openmax_probs", "otal_decode_clips_openmax")


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "openmax.npz"))


@pytest.fixture(scope="module")
def lib():
    from opental_amd.csrc import build
    if not os.path.exists(build.LIB):
        build.build(verbose=False)
    from opental_amd._lib import declare
    return declare(ctypes.CDLL(build.LIB))


def fits_of(fx, stage):
    p = fx["fit_params"][stage * K:(stage + 1) * K]
    return dict(scale=p[:, 0], shape=p[:, 1], small=p[:, 2])


def test_openmax_symbols_are_exported_and_declared(lib):
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "opental_hip.h")).read()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert f"int {name}(" in header, name
    assert lib.otal_abi_version() == 26


def test_openmax_argument_errors_do_not_launch(lib):
    one = ctypes.c_void_p(16)           # never dereferenced: argument checks come first
    dist = lambda feat, n, rpb, mav, k, d, out: lib.otal_openmax_dist(feat, n, rpb, 0, d, 1, mav, k, d, None, out, None)
    assert dist(None, 4, 4, one, 15, 512, one) == -1
    assert dist(one, 4, 4, one, 15, 512, None) == -1
    assert dist(one, 0, 4, one, 15, 512, one) == -2
    assert dist(one, 4, 0, one, 15, 512, one) == -2
    assert dist(one, 4, 4, one, 17, 512, one) == -7             # more classes than a workgroup stages
    assert dist(one, 4, 4, one, 15, 516, one) == -7             # D beyond the staged row
    assert dist(one, 4, 4, one, 15, 504, one) == -7             # D % 16
    assert dist(one, 4, 4, ctypes.c_void_p(20), 15, 512, one) == -7        # MAVs not 16-byte aligned
    means = lambda feat, lab, n, k, out, cnt: lib.otal_openmax_class_means(feat, n, n, 0, 512, 1, lab, k, 512, out, cnt, None)
    assert means(one, None, 4, 15, one, one) == -1
    assert means(one, one, 4, 15, one, None) == -1
    assert means(one, one, 4, 0, one, one) == -2
    probs = lambda logits, ldl, wb, k, r, out: lib.otal_openmax_probs(logits, ldl, one, 4, 4, 0, 512, 1, one, wb,
                                                                     k, 512, r, out, None)
    assert probs(None, 15, one, 15, 1, one) == -1
    assert probs(one, 15, None, 15, 1, one) == -1
    assert probs(one, 14, one, 15, 1, one) == -2                # logit rows shorter than K
    assert probs(one, 15, one, 15, 0, one) == -7                # rank outside [1, K]
    assert probs(one, 15, one, 15, 16, one) == -7
    st = (ctypes.c_int64 * 3)(A * 512, 512, 1)

    def decode(loc=one, feat=one, prop_feat=None, pst=None, unknown=one, n=2, c=16, first=1, d=512, r=1, refined=0):
        return lib.otal_decode_clips_openmax(loc, one, one, one, one, one, one, one, feat, prop_feat, st, pst, one, one, one, one,
                                             one, one, unknown, one, n, A, c, first, d, r, refined, 256.0, 0.01, None)
    assert decode(loc=None) == -1
    assert decode(feat=None) == -1
    assert decode(unknown=None) == -1
    assert decode(refined=1) == -1                              # the refined feature is asked for but not given
    assert decode(n=0) == -2
    assert decode(c=1) == -2                                    # nothing left once the background logit is dropped
    assert decode(c=18) == -7
    assert decode(d=1024) == -7
    assert decode(r=0) == -7
    assert decode(r=16) == -7
    assert decode(refined=2, prop_feat=one, pst=st) == -7
    # the softmax / Dirichlet decode keeps refusing a third score function: OpenMax has entries of its own
    assert lib.otal_decode_clips_ex(one, one, one, one, one, one, None, None, one, one, one, one, None, None, one, 2, A, 16,
                                    256.0, 0.01, 2, 1, None) == -7


def test_weibull_fit_matches_libmr_within_its_stopping_error(fx):
    """weibull_fit_high on the golden tails against libMR's w_score on the golden grid.  libMR stops its root finder at 1e-6;
    the pin tool recorded max |w_libMR - w_exact MLE| over the fixture (`fit_dev`, extended-precision MLE of
    tests/openmax_ref.py); 4x that is allowed -- the factor covers which side of the root libMR lands on."""
    from opental_amd.thumos14.openmax import weibull_fit_high
    bound = 4 * float(fx["fit_dev"])
    assert 0 < bound < 1e-5
    worst = 0.0
    for tail, grid, w, par in zip(fx["fit_tails"], fx["fit_grid"], fx["fit_w"], fx["fit_params"]):
        fit = weibull_fit_high(tail)
        assert fit.small_score == par[2] == tail.min()
        assert fit.translate == 10000.0
        worst = max(worst, float(np.abs(fit.w_score(grid) - w).max()))
        assert isinstance(fit.w_score(float(grid[3])), float)
    print(f"max |w_fit - w_libMR| = {worst:.3e} (bound {bound:.3e})")
    assert worst <= bound


def test_weibull_fit_equals_the_extended_precision_mle(fx):
    from opental_amd.thumos14.openmax import weibull_fit_high
    for tail in fx["fit_tails"]:
        fit = weibull_fit_high(tail[::-1].astype(np.float32).astype(np.float64))       # any order, float32-valued
        scale, shape, small = R.weibull_mle_exact(tail)
        assert fit.small_score == small
        assert abs(fit.scale - scale) <= 1e-12 * scale and abs(fit.shape - shape) <= 1e-9 * shape


def test_degenerate_tails_raise_and_name_the_class():
    from opental_amd.thumos14.openmax import weibull_fit_high
    for tail in ([0.5] * 20, [0.3], [], [0.2, float('nan')]):
        with pytest.raises(ValueError, match="Diving"):
            weibull_fit_high(tail, "Diving")


def test_stable_float32_w_score_form(fx):
    """The form the kernel evaluates, in float32 numpy on float64-prepared constants, stays within 4e-6 of libMR's float64
    w_score on the golden grid, where the literal float32 formula is off by more than 1e-3."""
    p = fx["fit_params"]
    wb = R.w_constants(p[:, 0], p[:, 1], p[:, 2]).astype(np.float32)
    stable = R.w_score32_stable(fx["fit_grid"].astype(np.float32), wb[:, None, :])
    exact = np.stack([R.w_score64(g.astype(np.float32), *q) for g, q in zip(fx["fit_grid"], p)])
    literal = R.w_score32_literal(fx["fit_grid"], p[:, :1], p[:, 1:2], p[:, 2:3])
    assert np.abs(stable - exact).max() < 4e-6
    assert np.abs(literal - exact).max() > 1e-3
    from opental_amd.thumos14.openmax import WeibullFit
    for q, row in zip(p, wb):
        assert np.array_equal(np.asarray(WeibullFit(*q).device_constants(), np.float64).astype(np.float32), row)


def test_float64_restatement_equals_the_golden(fx):
    """Pins the checker (tests/openmax_ref.py), not the product: items 1, 3 and 4 of the reference in float64."""
    labels = R.stat_labels()
    for tag, cs, fs in (("", "centres", "stat"), ("_prop", "prop_centres", "prop_stat")):
        feats = R.features_of(R.class_centres(int(fx["seed_" + cs])), labels, int(fx["seed_" + fs]))
        mav = np.stack([feats[labels == k].mean(0) for k in range(K)])
        assert mav.dtype == np.float32
        np.testing.assert_allclose(mav, fx["mav" + tag], rtol=1e-6)             # float32 means in numpy's order
        d = R.eucos(fx["mav" + tag], feats)[np.arange(len(labels)), labels]
        np.testing.assert_allclose(d, fx["dist" + tag], rtol=1e-9)
    lab = fx["rows_labels"].astype(np.int64)
    seed = int(fx["seed_rows"])
    assert np.array_equal(np.random.RandomState(seed).randint(0, K, 256), lab)
    feats = R.features_of(R.class_centres(int(fx["seed_centres"])), lab, seed + 1)
    logits = R.logits_of(lab, seed + 2)
    for rank in (1, 3):
        p = R.openmax_probs(logits, feats, fx["mav"], fits_of(fx, 0), rank)
        np.testing.assert_allclose(p, fx[f"probs_r{rank}"], rtol=1e-9, atol=1e-300)
    outs = R.clip_outputs(int(fx["decode_seed"]), R.class_centres(int(fx["seed_centres"])), R.class_centres(int(fx["seed_prop_centres"])))
    seg, score = R.decode(outs, fx["clips"], fx["mav"], fits_of(fx, 0), fx["mav_prop"], fits_of(fx, 1))
    np.testing.assert_allclose(score, fx["decode_score"], rtol=1e-9, atol=1e-300)
    np.testing.assert_allclose(seg, fx["decode_seg"], rtol=1e-6, atol=1e-6)
    assert np.array_equal(score > fx["decode_params"][0], fx["decode_mask"].astype(bool))
    _, refined = R.decode(outs, fx["clips"], fx["mav"], fits_of(fx, 0), fx["mav_prop"], fits_of(fx, 1), refined_feature=True)
    assert np.abs(refined - fx["decode_score"]).max() > 1e-2


def test_fixture_keeps_clear_of_the_threshold_and_of_ties(fx):
    """What the pin tool asserted when it chose the decode seed."""
    tol = 4 * float(fx["tol_score"][0])
    s = fx["decode_score"][:, 1:]
    assert (np.abs(s - fx["decode_params"][0]) <= tol).sum() < 0.01 * s.size
    for cl in range(K):
        v = np.sort(s[:, cl][s[:, cl] > fx["decode_params"][0]])
        assert v.size < 2 or np.diff(v).min() > 10 * tol
    for rank in (1, 3):
        lab = fx["rows_labels"].astype(np.int64)
        z = R.logits_of(lab, int(fx["seed_rows"]) + 2)
        assert all(len(set(row)) == K for row in z.tolist())            # no ties in the ranked logits


def test_mav_dist_files_round_trip_with_the_reference_keys(fx, tmp_path):
    from opental_amd.thumos14 import test_openmax as TO
    from opental_amd.thumos14.openmax import weibull_fit_high
    labels = R.stat_labels()
    idx_to_class = {i + 1: n for i, n in enumerate(NAMES)}
    t = lambda a, dt=torch.float32: torch.from_numpy(np.asarray(a)).to(dt)
    stats = lambda tag: (t(fx["mav" + tag]), t(np.full(K, 40), torch.int32), t(fx["dist" + tag].astype(np.float32)), t(labels, torch.int32))
    TO.save_mav_dist(str(tmp_path / "mav_dist"), idx_to_class, stats(""), stats("_prop"))
    assert TO.files_are_ready(str(tmp_path / "mav_dist"), idx_to_class)
    data = np.load(str(tmp_path / "mav_dist" / "class_3.npz"))
    assert sorted(data.files) == ["dist", "dist_prop", "mav", "mav_prop"]
    assert np.array_equal(data["mav"], fx["mav"][2]) and data["dist"].shape == (40,) and data["mav_prop"].shape == (D,)
    models = TO.weibull_fitting(idx_to_class, str(tmp_path / "mav_dist"), tailsize=20)
    for stage, model in enumerate(models):
        assert list(model) == NAMES
        for k, name in enumerate(NAMES):
            want = weibull_fit_high(fx["fit_tails"][stage * K + k])
            got = model[name]['model'][0]
            assert (got.scale, got.shape, got.small_score) == (want.scale, want.shape, want.small_score)
            assert np.array_equal(model[name]['mean_vec'], fx["mav" + ("_prop" if stage else "")][k])
    # a class without a positive anchor: a clear error, not np.stack([])
    counts = np.full(K, 40)
    counts[6] = 0
    bad = (t(fx["mav"]), t(counts, torch.int32), t(fx["dist"].astype(np.float32)), t(labels, torch.int32))
    with pytest.raises(ValueError, match="class_7"):
        TO.save_mav_dist(str(tmp_path / "bad"), idx_to_class, bad, stats("_prop"))
    assert not TO.files_are_ready(str(tmp_path / "bad"), idx_to_class)


def test_get_matched_targets_equals_the_reference_labels(fx):
    from opental_amd.thumos14.test_openmax import get_matched_targets
    loc, targets = R.match_inputs(int(fx["seed_match"]))
    loc_t, conf_t, prop_loc_t, prop_conf_t = get_matched_targets([torch.from_numpy(t) for t in targets], torch.from_numpy(loc),
                                                                 torch.from_numpy(R.priors()), 256, 0.5)
    assert conf_t.dtype == torch.long and loc_t.shape == (3, A, 2) and prop_loc_t.shape == (3, A, 2)
    assert np.array_equal(conf_t.numpy(), fx["match_conf_t"])
    assert np.array_equal(prop_conf_t.numpy(), fx["match_prop_conf_t"])


def test_openmax_layer_has_no_cpu_fallback(fx):
    from opental_amd.thumos14.openmax import OpenMax, compute_eucos_dist, weibull_fit_high
    model = {n: {'mean_vec': fx["mav"][k], 'model': [weibull_fit_high(fx["fit_tails"][k], n)]} for k, n in enumerate(NAMES)}
    layer = OpenMax(model, rank=3)
    assert layer.num_cls == K and layer.rank == 3 and layer.class_names == NAMES
    assert OpenMax(model, rank=99).rank == K                    # openmax.py:47
    with pytest.raises(ValueError):
        OpenMax(model, rank=0)
    with pytest.raises(RuntimeError):
        layer(torch.zeros(4, K), torch.zeros(4, D))
    with pytest.raises(RuntimeError):
        compute_eucos_dist(torch.zeros(K, D), torch.zeros(4, D))
    big = {f"c{i}": model[NAMES[0]] for i in range(17)}
    with pytest.raises(NotImplementedError):
        OpenMax(big)
