"""tools/pin_openmax_wide.py -- fixture generator for the ActivityNet1.3 OpenMax baseline (K = 150 classes); runs where the
reference source tree is available, never on the GPU machine.

Follows tools/pin_openmax.py and uses its pieces: the reference's libMR compiled behind tools/libmr_shim.cpp into
oracle/_ref/ (git-ignored), a stand-in `libmr` module over it, the reference's openmax.py and test_openmax.py imported after
oracle.pin_against_reference.import_reference().  The reference is fed float64 tensors holding float32 values, so the golden
is its arithmetic without float32 noise.  Inputs come from the seeds stored in the file and tests/openmax_wide_ref.py; the MAVs
are the seeded class centres themselves, so none are stored.

Recorded at K = 150, D = 512:
  (a) fits  -- 2 x 150 tails of 20 own-class distances (float32-rounded, as the reference produces them) of 40 rows per class,
               libMR's (scale, shape, small_score) for them through the reference's weibull_fitting, and `fit_dev`, the largest
               |w(libMR parameters) - w(extended-precision MLE)| on the 41-point grids of openmax_wide_ref.fit_grid (libMR
               stops its root finder at 1e-6): the CPU test allows 4x that;
  (b) probs -- the reference OpenMax.forward with rank 1 and rank 3 on 64 rows;
  (c) decode-- n = 2 clips, A = 189 (ActivityNet priors with level ids), C = 151, clip_length 768, conf_thresh 0.001:
               probabilities from the reference layers (the refined stage's layer reads the coarse feature, as the reference
               ships it), averaged and scaled as decode_output does (thumos14/test_openmax.py:158-164); segments by the
               arithmetic of anet/test.py:110-115 and `filtering`'s (segment + offset) / fps in float32.  The float64 scores
               are stored for the anchors openmax_wide_ref.DECODE_ANCHORS (every third: the full (2, 151, 189) array does not
               fit), the threshold mask for every cell.
`tol_probs_r1`, `tol_probs_r3`, `tol_score`, `tol_unknown`, `tol_dist`, `tol_dist_prop`: [largest absolute, largest relative]
deviation of the float32 numpy restatement (tests/openmax_ref.py, stable w-score form) from the reference; the GPU tests
allow 4x the absolute one.  Asserted here: at most 1 % of the decode case's (clip, class, anchor) cells have a float64 score
within 4 * tol_score of conf_thresh (if more do, change SEEDS['decode']; do not raise the cap).

Writes tests/golden/openmax_wide.npz and tests/golden/PIN_REPORT_openmax_wide.txt.

    python -m tools.pin_openmax_wide
"""
import os
import sys
import tempfile
import types

sys.dont_write_bytecode = True
os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np
import torch

import openmax_ref as R
import openmax_wide_ref as W
from oracle.pin_against_reference import REF, import_reference
from tools.pin_openmax import GOLD, build_libmr, dev, fake_libmr

K, D, A = W.K, W.D, W.A
SEEDS = dict(centres=301, prop_centres=302, stat=303, prop_stat=304, rows=305, decode=306)
CLIPS = ((0.0, 5.0), (0.0, 7.0))            # (offset, fps): an ActivityNet video is one clip at offset 0
CONF_THRESH = 0.001
MAX_BYTES = 450 * 1024


def pin_fits(ref_openmax, ref_tom, res, report):
    stats = []
    for tag, cseed, fseed in (("", SEEDS['centres'], SEEDS['stat']), ("_prop", SEEDS['prop_centres'], SEEDS['prop_stat'])):
        cen = R.class_centres(cseed, K, D)
        feats, labels = W.stat_rows(cen, fseed)
        dist = np.array([ref_openmax.compute_eucos_dist(cen[l].astype(np.float64), f.astype(np.float64))
                         for l, f in zip(labels, feats)])
        d32 = W.eucos_own(cen[labels], feats, np.float32)
        res["tol_dist" + tag] = dev(d32, dist)
        np.testing.assert_allclose(W.eucos_own(cen[labels], feats), dist, rtol=1e-9)
        report.append(f"stats{tag}: {len(labels)} rows against the centre of their class; dist in [{dist.min():.4f}, "
                      f"{dist.max():.4f}]; float32 restatement abs {res['tol_dist' + tag][0]:.3e} rel {res['tol_dist' + tag][1]:.3e}")
        stats.append((cen, dist.astype(np.float32).astype(np.float64), labels))
    with tempfile.TemporaryDirectory() as d:
        (cen, dist, lab), (pcen, pdist, plab) = stats
        for k, name in enumerate(W.NAMES):
            np.savez(os.path.join(d, f"{name}.npz"), mav=cen[k], dist=dist[lab == k], mav_prop=pcen[k], dist_prop=pdist[plab == k])
        cfg = types.SimpleNamespace(idx_to_class={i + 1: n for i, n in enumerate(W.NAMES)})
        models = ref_tom.weibull_fitting(cfg, d, tailsize=W.TAILSIZE)
    tails, par, worst = [], [], 0.0
    for model, (cen, dist, lab) in zip(models, stats):
        tl = W.tails_of(dist, lab)
        for k, name in enumerate(W.NAMES):
            mr = model[name]['model'][0]
            g = W.fit_grid(tl[k])
            wl = np.array([mr.w_score(x) for x in g])
            assert np.abs(wl - R.w_score64(g, mr.scale, mr.shape, mr.small_score)).max() < 1e-12      # w_score is this formula
            sc, sh, sm = R.weibull_mle_exact(tl[k])
            assert sm == mr.small_score == tl[k].min()
            worst = max(worst, float(np.abs(wl - R.w_score64(g, sc, sh, sm)).max()))
            par.append([mr.scale, mr.shape, mr.small_score])
            model[name]['mean_vec'] = np.asarray(model[name]['mean_vec'], np.float64)      # the reference then runs in float64
        tails.append(tl)
    res.update(fit_tails=np.concatenate(tails), fit_params=np.array(par), fit_dev=np.array(worst))
    par = np.array(par)
    report.append(f"fits: {len(par)} tails of {W.TAILSIZE}; libMR shape in [{par[:, 1].min():.4g}, {par[:, 1].max():.4g}]; max "
                  f"|w_libMR - w_exact MLE| on the grids = {worst:.3e} (the CPU test allows 4x)")
    return models


def pin_probs(ref_openmax, models, res, report):
    feats, logits, lab = W.prob_rows(res)
    assert all(len(set(row)) == K for row in logits.tolist())                   # no ties in the ranked logits
    mav = W.mavs(res)[0]
    for rank in (1, 3):
        layer = ref_openmax.OpenMax(models[0], rank=rank)
        p = layer(torch.from_numpy(logits.astype(np.float64)), torch.from_numpy(feats.astype(np.float64))).numpy()
        assert p.dtype == np.float64 and p.shape == (64, K + 1)
        res[f"probs_r{rank}"] = p
        np.testing.assert_allclose(R.openmax_probs(logits, feats, mav, W.fits_of(res, 0), rank), p, rtol=1e-9, atol=1e-300)
        p32 = R.openmax_probs(logits, feats, mav, W.fits_of(res, 0), rank, np.float32)
        res[f"tol_probs_r{rank}"] = dev(p32, p)
        moved = np.abs(p[:, 1:] - R.recalibrate(logits, None, np.zeros_like(logits, np.float64), rank)[:, 1:]).max()
        report.append(f"probs rank {rank}: 64 rows; P(unknown) in [{p[:, 0].min():.3g}, {p[:, 0].max():.3g}]; the recalibration "
                      f"moves a class probability by up to {moved:.3g}; float32 restatement abs {res[f'tol_probs_r{rank}'][0]:.3e} "
                      f"rel {res[f'tol_probs_r{rank}'][1]:.3e}")


def pin_decode(ref_openmax, models, res, report):
    cen, pcen = W.mavs(res)
    outs = W.clip_outputs(SEEDS['decode'], cen, pcen, 2)
    layers = ref_openmax.OpenMax(models[0]), ref_openmax.OpenMax(models[1])
    f64 = lambda a: torch.from_numpy(a.astype(np.float64))
    scores = []
    for i in range(2):
        conf = layers[0](f64(outs['conf'][i][:, 1:]), f64(outs['conf_feat'][i]))
        prop_conf = layers[1](f64(outs['prop_conf'][i][:, 1:]), f64(outs['conf_feat'][i]))     # the coarse feature, as shipped
        center = torch.from_numpy(outs['center'][i]).sigmoid()
        conf = (conf + prop_conf) / 2.0
        conf = conf * center
        scores.append(conf.view(-1, K + 1).transpose(1, 0).numpy().copy())
    scores = np.stack(scores)
    assert scores.dtype == np.float64 and scores.shape == (2, K + 1, A)
    args = (cen, W.fits_of(res, 0), pcen, W.fits_of(res, 1))
    np.testing.assert_allclose(W.decode(outs, *args), scores, rtol=1e-9, atol=1e-300)
    s32 = W.decode(outs, *args, dt=np.float32)
    tol_score, tol_unk = dev(s32[:, 1:], scores[:, 1:]), dev(s32[:, 0], scores[:, 0])
    total = scores[:, 1:].size
    near = int((np.abs(scores[:, 1:] - CONF_THRESH) <= 4 * tol_score[0]).sum())
    assert near <= 0.01 * total, f"{near} of {total} scores within 4 * tol_score of the threshold: change SEEDS['decode']"
    refined = W.decode(outs, *args, refined_feature=True)
    res.update(clips=np.array(CLIPS, np.float64), decode_params=np.array([CONF_THRESH, W.CLIP_LENGTH], np.float64),
               decode_anchors=W.DECODE_ANCHORS.astype(np.int16), decode_score=scores[:, :, W.DECODE_ANCHORS],
               decode_mask=(scores > CONF_THRESH).astype(np.uint8), decode_seg=W.segments(outs, CLIPS),
               tol_score=tol_score, tol_unknown=tol_unk)
    report.append(f"decode: seed {SEEDS['decode']}; {int(res['decode_mask'][:, 1:].sum())} of {total} scores pass the threshold "
                  f"{CONF_THRESH}, {near} lie within 4 * tol_score = {4 * tol_score[0]:.3e} of it (cap: 1 % = {total // 100}); "
                  f"float64 scores stored for {len(W.DECODE_ANCHORS)} of {A} anchors; float32 restatement: score abs "
                  f"{tol_score[0]:.3e} rel {tol_score[1]:.3e}, unknown abs {tol_unk[0]:.3e} rel {tol_unk[1]:.3e}; with the refined "
                  f"feature in the refined stage the scores move by up to {np.abs(refined - scores).max():.3e}")


def main():
    torch.manual_seed(0)
    fake_libmr(build_libmr())
    _, _, _, _, ref_test = import_reference()
    sys.modules["test"] = ref_test                      # test_openmax.py: `from test import prepare_data, ...`
    sys.path.insert(0, os.path.join(REF, "AFSD", "thumos14"))
    import openmax as ref_openmax
    import test_openmax as ref_tom
    res = {f"seed_{k}": np.array(v) for k, v in SEEDS.items()}
    report = ["OpenMax fixtures at K = 150 (tools/pin_openmax_wide.py): reference openmax.py / test_openmax.py imported after "
              "import_reference(); libMR = the reference's MetaRecognition.cpp + weibull.c behind tools/libmr_shim.cpp; the "
              "reference runs in float64 on float32-valued inputs; MAVs are the seeded class centres"]
    models = pin_fits(ref_openmax, ref_tom, res, report)
    pin_probs(ref_openmax, models, res, report)
    pin_decode(ref_openmax, models, res, report)
    path = os.path.join(GOLD, "openmax_wide.npz")
    np.savez_compressed(path, **res)
    size = os.path.getsize(path)
    report.append(f"tests/golden/openmax_wide.npz: {size} bytes")
    assert size < MAX_BYTES, size
    with open(os.path.join(GOLD, "PIN_REPORT_openmax_wide.txt"), "w") as f:
        f.write("\n".join(report) + "\n")
    print("\n".join(report))
    leftovers = [os.path.join(d_, n) for d_, _, fs in os.walk(REF) for n in fs if n.endswith(".pyc")]
    assert not leftovers, leftovers


if __name__ == "__main__":
    main()
