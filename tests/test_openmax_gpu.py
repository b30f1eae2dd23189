"""GPU: the OpenMax baseline's kernels (csrc/openmax.hip) and inference path against tests/golden/openmax.npz, which
tools/pin_openmax.py recorded from the reference (its openmax.py / test_openmax.py over libMR, in float64).

Tolerances.  For dist, class means, probabilities, scores and `unknown` the pin tool evaluated a plain float32 numpy
restatement (tests/openmax_ref.py, stable w-score form) and stored its largest absolute deviation from the reference as
`tol_*`; every assertion here allows 4x that figure -- the margin covers the device's expf / logf / log1pf and another order
of the 512-term sums.  No kernel is compared with itself or with the package's own torch code; where the golden holds only a
subset (own-class distances), the rest is checked against the float64 restatement that tests/test_openmax_cpu.py pins to the
golden.  Each test prints its figures before it asserts."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch
import yaml

import openmax_ref as R
from oracle import arch

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, D, A = R.K, R.D, R.A
NAMES = [f"class_{i}" for i in range(1, K + 1)]
GUARD = 4096
SENTINEL_F32 = 0x7F7FBEEF       # as tests/test_conv_calls_gpu.py: a finite pattern nobody writes by accident
SENTINEL_U8 = 0xA5


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "openmax.npz"))


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def fits_of(fx, stage):
    p = fx["fit_params"][stage * K:(stage + 1) * K]
    return dict(scale=p[:, 0], shape=p[:, 1], small=p[:, 2])


def layers(fx, rank=1):
    """The two OpenMax layers from the golden MAVs and tails, fitted by the package's float64 weibull_fit_high (pinned to libMR
    by tests/test_openmax_cpu.py)."""
    from opental_amd.thumos14.openmax import OpenMax, weibull_fit_high
    out = []
    for stage, tag in enumerate(("", "_prop")):
        model = {n: {'mean_vec': fx["mav" + tag][k], 'model': [weibull_fit_high(fx["fit_tails"][stage * K + k], n)]}
                 for k, n in enumerate(NAMES)}
        out.append(OpenMax(model, rank=rank))
    return out


def stat_rows(fx, tag=""):
    labels = R.stat_labels()
    cs, fs = ("prop_centres", "prop_stat") if tag else ("centres", "stat")
    return R.features_of(R.class_centres(int(fx["seed_" + cs])), labels, int(fx["seed_" + fs])), labels


def prob_rows(fx):
    lab = fx["rows_labels"].astype(np.int64)
    seed = int(fx["seed_rows"])
    return R.features_of(R.class_centres(int(fx["seed_centres"])), lab, seed + 1), R.logits_of(lab, seed + 2)


def clip_outs(fx, dev):
    outs = R.clip_outputs(int(fx["decode_seed"]), R.class_centres(int(fx["seed_centres"])), R.class_centres(int(fx["seed_prop_centres"])))
    t = {k: torch.from_numpy(v).to(dev) for k, v in outs.items()}
    t['priors'] = torch.from_numpy(R.priors()).to(dev)
    return outs, t


def worst(got, want):
    return float(np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64)).max())


def channel_major_view(t):
    """(B, A, D) or (N, D) values held channel-major, as the towers produce them: a permuted view, not a copy."""
    v = t.transpose(-1, -2).contiguous().transpose(-1, -2)
    assert not v.is_contiguous() and v.stride(-2) == 1 and torch.equal(v, t)
    return v


# ----------------------------------------------------------------------------- statistics kernels
@pytest.mark.parametrize("tag", ["", "_prop"])
def test_dist_matches_the_reference(fx, dev, tag):
    from opental_amd.thumos14.openmax import compute_eucos_dist
    feats, labels = stat_rows(fx, tag)
    bound = 4 * float(fx["tol_dist" + tag][0])
    mav = torch.from_numpy(fx["mav" + tag]).to(dev)
    f = torch.from_numpy(feats).to(dev)
    own = compute_eucos_dist(mav, f, torch.from_numpy(labels).to(dev)).cpu().numpy()
    full = compute_eucos_dist(mav, f).cpu().numpy()
    assert own.shape == (600,) and full.shape == (600, K)
    e_own, e_full = worst(own, fx["dist" + tag]), worst(full, R.eucos(fx["mav" + tag], feats))
    print(f"dist{tag}: own-class max abs err {e_own:.3e}, all classes {e_full:.3e}, bound {bound:.3e}")
    assert e_own <= bound and e_full <= bound
    assert np.array_equal(full[np.arange(600), labels], own)
    lab = torch.from_numpy(labels).to(dev).clone()
    lab[5], lab[17] = -1, K
    marked = compute_eucos_dist(mav, f, lab).cpu().numpy()
    assert marked[5] == -1 and marked[17] == -1 and np.array_equal(np.delete(marked, [5, 17]), np.delete(own, [5, 17]))
    one = compute_eucos_dist(mav[3], f[:7]).cpu().numpy()           # a single MAV (D,): openmax.py:7-9 itself
    assert one.shape == (7, 1) and np.array_equal(one[:, 0], full[:7, 3])


@pytest.mark.parametrize("tag", ["", "_prop"])
def test_class_means_match_the_reference_and_are_deterministic(fx, dev, tag):
    from opental_amd.thumos14.openmax import class_means
    feats, labels = stat_rows(fx, tag)
    bound = 4 * float(fx["tol_mean" + tag][0])
    f = torch.from_numpy(feats).to(dev)
    lab = torch.from_numpy(labels).to(dev)
    mav, counts = class_means(f, lab, K)
    err = worst(mav.cpu().numpy(), fx["mav" + tag])
    print(f"class means{tag}: max abs err {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    assert counts.cpu().tolist() == [40] * K
    for _ in range(2):
        again, c2 = class_means(f, lab, K)
        assert torch.equal(again, mav) and torch.equal(c2, counts)
    strided, _ = class_means(channel_major_view(f), lab, K)
    assert torch.equal(strided, mav)
    lab2 = lab.clone()
    lab2[lab2 == 4] = -1                    # ignored rows; a class without rows has mean 0 and count 0
    m2, c2 = class_means(f, lab2, K)
    assert int(c2[4]) == 0 and float(m2[4].abs().max()) == 0.0 and torch.equal(m2[5], mav[5])


def test_statistics_pipeline_on_labelled_rows(fx, dev):
    """mav_and_dist = the two kernels in sequence (the distances see the kernel's own means, so only the yardstick of the
    means' deviation can be applied: a mean off by e moves a distance by at most ~e * sqrt(D) / 200 + 2 e sqrt(D) / |mav|)."""
    from opental_amd.thumos14.test_openmax import mav_and_dist
    feats, labels = stat_rows(fx)
    mav, counts, dist = mav_and_dist(torch.from_numpy(feats).to(dev), torch.from_numpy(labels).to(dev).int(), K)
    e = 4 * float(fx["tol_mean"][0])
    bound = 4 * float(fx["tol_dist"][0]) + e * np.sqrt(D) / 200 + 2 * e * np.sqrt(D) / float(np.linalg.norm(fx["mav"], axis=1).min())
    err = worst(dist.cpu().numpy(), fx["dist"])
    print(f"pipeline dist: max abs err {err:.3e}, bound {bound:.3e}")
    assert err <= bound and counts.sum().item() == 600


# ----------------------------------------------------------------------------- OpenMax.forward
@pytest.mark.parametrize("rank", [1, 3])
def test_openmax_forward_matches_the_reference(fx, dev, rank):
    feats, logits = prob_rows(fx)
    layer = layers(fx, rank)[0].to(dev)
    bound = 4 * float(fx[f"tol_probs_r{rank}"][0])
    f, z = torch.from_numpy(feats).to(dev), torch.from_numpy(logits).to(dev)
    p = layer(z, f)
    assert p.shape == (256, K + 1) and p.dtype == torch.float32 and p.is_cuda
    err = worst(p.cpu().numpy(), fx[f"probs_r{rank}"])
    print(f"probs rank {rank}: max abs err {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    assert abs(float(p.sum(1).max()) - 1) < 1e-5
    # both layouts give the same bits; so does a `conf[:, 1:]` view of logits that carry a background column
    assert torch.equal(layer(z, channel_major_view(f)), p)
    wide = torch.cat([torch.full((256, 1), 9.0, device=dev), z], 1)
    assert torch.equal(layer(wide[:, 1:], f), p)
    # a row count that is no multiple of the 16-row tile
    assert torch.equal(layer(z[:37], f[:37]), p[:37])


def test_rank_ties_take_the_higher_index_first(fx, dev):
    """`argsort()[::-1]` of equal logits lists the higher index first: with rank 1 and logits 3 == 7 tied at the top, class 7
    (0-based) is the one recalibrated.  The golden holds no ties, so this is checked against the float64 restatement."""
    feats, logits = prob_rows(fx)
    logits = logits[:32].copy()
    logits[:, 3] = logits[:, 7] = logits.max(1) + 1.0
    assert (np.argsort(logits, 1)[:, -1] == 7).all()
    layer = layers(fx, 1)[0].to(dev)
    p = layer(torch.from_numpy(logits).to(dev), torch.from_numpy(feats[:32]).to(dev)).cpu().numpy()
    want = R.openmax_probs(logits, feats[:32], fx["mav"], fits_of(fx, 0), 1)
    assert worst(p, want) <= 4 * float(fx["tol_probs_r1"][0])
    assert np.abs(want[:, 1 + 3] - want[:, 1 + 7]).max() > 1e-3           # the two tied classes do come out differently


# ----------------------------------------------------------------------------- the decode launch
def test_decode_matches_the_reference(fx, dev):
    from opental_amd.thumos14.test_openmax import decode_clips_openmax
    _, t = clip_outs(fx, dev)
    lay = [l.to(dev) for l in layers(fx)]
    thr = float(fx["decode_params"][0])
    dec = decode_clips_openmax(t, fx["clips"][:, 0].tolist(), fx["clips"][:, 1].tolist(), lay[0], lay[1], 256, thr)
    assert dec['unct'] is None and dec['actn'] is None and dec['score'].shape == (2, K, A) and dec['flag'].dtype == torch.uint8
    b_score, b_unk = 4 * float(fx["tol_score"][0]), 4 * float(fx["tol_unknown"][0])
    score, ref = dec['score'].cpu().numpy(), fx["decode_score"]
    e_score, e_unk = worst(score, ref[:, 1:]), worst(dec['unknown'].cpu().numpy(), ref[:, 0])
    print(f"decode: score max abs err {e_score:.3e} (bound {b_score:.3e}), unknown {e_unk:.3e} (bound {b_unk:.3e})")
    assert e_score <= b_score and e_unk <= b_unk
    np.testing.assert_allclose(dec['seg'].cpu().numpy(), fx["decode_seg"], rtol=1e-6, atol=1e-5)
    close = np.abs(ref[:, 1:] - thr) <= b_score
    assert close.sum() <= 0.01 * close.size
    flag = dec['flag'].cpu().numpy()
    assert np.array_equal(flag[~close], fx["decode_mask"][:, 1:][~close])
    assert np.array_equal(flag.astype(bool), score > thr)
    # deterministic, and the same bits from channel-major feature views
    again = decode_clips_openmax(t, fx["clips"][:, 0].tolist(), fx["clips"][:, 1].tolist(), lay[0], lay[1], 256, thr)
    t2 = dict(t, conf_feat=channel_major_view(t['conf_feat']), prop_conf_feat=channel_major_view(t['prop_conf_feat']))
    strided = decode_clips_openmax(t2, fx["clips"][:, 0].tolist(), fx["clips"][:, 1].tolist(), lay[0], lay[1], 256, thr)
    for k in ('seg', 'score', 'unknown', 'flag'):
        assert torch.equal(again[k], dec[k]) and torch.equal(strided[k], dec[k]), k
    # the decode launch is the two OpenMax.forward launches + the average: the shared recalibration gives the same bits
    p0 = lay[0](t['conf'][0][:, 1:], t['conf_feat'][0])
    p1 = lay[1](t['prop_conf'][0][:, 1:], t['conf_feat'][0])
    ct = 1.0 / (1.0 + torch.exp(-t['center'][0]))
    np.testing.assert_allclose(((p0 + p1) / 2.0 * ct).t()[1:].cpu().numpy(), score[0], rtol=1e-6, atol=1e-9)


def test_refined_feature_switch_is_live(fx, dev):
    from opental_amd.thumos14.test_openmax import decode_clips_openmax
    outs, t = clip_outs(fx, dev)
    lay = [l.to(dev) for l in layers(fx)]
    args = (fx["clips"][:, 0].tolist(), fx["clips"][:, 1].tolist(), lay[0], lay[1], 256, float(fx["decode_params"][0]))
    dec = decode_clips_openmax(t, *args, refined_feature=True)
    score = dec['score'].cpu().numpy()
    assert worst(score, fx["decode_score"][:, 1:]) > 1e-2               # not what the reference ships
    _, want = R.decode(outs, fx["clips"], fx["mav"], fits_of(fx, 0), fx["mav_prop"], fits_of(fx, 1), refined_feature=True)
    err = worst(score, want[:, 1:])
    print(f"decode with the refined feature: max abs err {err:.3e} against the float64 restatement")
    assert err <= 4 * float(fx["tol_score"][0])
    again = decode_clips_openmax(t, *args, refined_feature=True)
    assert torch.equal(again['score'], dec['score']) and torch.equal(again['unknown'], dec['unknown'])


def test_detections_match_the_reference_list(fx, dev):
    from opental_amd.thumos14 import test as T
    from opental_amd.thumos14.test_openmax import decode_clips_openmax
    _, t = clip_outs(fx, dev)
    lay = [l.to(dev) for l in layers(fx)]
    thr, top_k, sigma = float(fx["decode_params"][0]), int(fx["decode_params"][1]), float(fx["decode_params"][2])
    offs, fps = fx["clips"][:, 0].tolist(), fx["clips"][:, 1].tolist()

    def detections(refined):
        dec = decode_clips_openmax(t, offs, fps, lay[0], lay[1], 256, thr, refined_feature=refined)
        rows, counts, _ = T.softnms_classes(dec, [0, 2], top_k, sigma)
        assert rows.shape[-1] == 3
        props = T.get_video_detections(rows[0], counts[0], None, top_k)
        assert all(p['uncertainty'] == 0.0 and p['actionness'] == 0.0 for p in props)
        return np.array([[p['label'], p['score'], p['segment'][0], p['segment'][1]] for p in props], np.float64).reshape(-1, 4)
    got, want = detections(False), fx["decode_detections"]
    assert got.shape == want.shape and np.array_equal(got[:, 0], want[:, 0])
    # the reference's rows are float32 (`res`, test_openmax.py:194): half an ulp of storage on top of the score yardstick
    bound = 4 * float(fx["tol_score"][0]) + 2.0 ** -24
    err = worst(got[:, 1], want[:, 1])
    print(f"detections: {len(got)} rows, score max abs err {err:.3e} (bound {bound:.3e})")
    assert err <= bound
    np.testing.assert_allclose(got[:, 2:], want[:, 2:], rtol=1e-6, atol=1e-5)
    other = detections(True)
    assert other.shape != want.shape or worst(other[:, 1], want[:, 1]) > 1e-3


# ----------------------------------------------------------------------------- output extent
def guarded(n, dev, dtype=torch.float32):
    """A sentinel-filled buffer with GUARD elements on either side of an n-element output view."""
    if dtype == torch.uint8:
        buf = torch.full((n + 2 * GUARD,), SENTINEL_U8, dtype=torch.uint8, device=dev)
    else:
        buf = torch.full((n + 2 * GUARD,), SENTINEL_F32, dtype=torch.int32, device=dev).view(dtype)
    return buf, buf[GUARD:GUARD + n]


def check_guard(buf, n, name, written_everywhere=True):
    raw = buf.view(torch.int32) if buf.dtype != torch.uint8 else buf
    s = SENTINEL_U8 if buf.dtype == torch.uint8 else SENTINEL_F32
    assert bool((raw[:GUARD] == s).all()) and bool((raw[GUARD + n:] == s).all()), f"{name}: wrote outside its output"
    if written_everywhere and buf.dtype != torch.uint8:
        assert not bool((raw[GUARD:GUARD + n] == s).any()), f"{name}: left part of its output unwritten"


@pytest.mark.parametrize("n_rows", [256, 37])
def test_launches_write_their_whole_output_and_nothing_else(fx, dev, n_rows):
    from opental_amd import _lib as L
    feats, logits = prob_rows(fx)
    f, z = torch.from_numpy(feats[:n_rows]).to(dev), torch.from_numpy(logits[:n_rows]).to(dev)
    lab = torch.from_numpy(fx["rows_labels"][:n_rows].astype(np.int32)).to(dev)
    lay = [l.to(dev) for l in layers(fx)]
    mav, wb = lay[0].tensors(dev)
    lib = L.lib()
    view = (n_rows, 0, D, 1)
    buf, out = guarded(n_rows * K, dev)
    L.check(lib.otal_openmax_dist(L.ptr(f), n_rows, *view, L.ptr(mav), K, D, None, L.ptr(out), L.stream()), "dist")
    check_guard(buf, n_rows * K, "otal_openmax_dist")
    buf, out = guarded(n_rows, dev)
    L.check(lib.otal_openmax_dist(L.ptr(f), n_rows, *view, L.ptr(mav), K, D, L.ptr(lab), L.ptr(out), L.stream()), "dist")
    check_guard(buf, n_rows, "otal_openmax_dist (labels)")
    buf, out = guarded(K * D, dev)
    cbuf, cnt = guarded(K, dev, torch.int32)
    L.check(lib.otal_openmax_class_means(L.ptr(f), n_rows, *view, L.ptr(lab), K, D, L.ptr(out), L.ptr(cnt), L.stream()), "means")
    check_guard(buf, K * D, "otal_openmax_class_means")
    check_guard(cbuf, K, "otal_openmax_class_means (counts)")
    buf, out = guarded(n_rows * (K + 1), dev)
    L.check(lib.otal_openmax_probs(L.ptr(z), K, L.ptr(f), n_rows, *view, L.ptr(mav), L.ptr(wb), K, D, 1, L.ptr(out),
                                   L.stream()), "probs")
    check_guard(buf, n_rows * (K + 1), "otal_openmax_probs")


@pytest.mark.parametrize("refined", [0, 1])
def test_decode_launch_writes_its_whole_output_and_nothing_else(fx, dev, refined):
    from opental_amd import _lib as L
    _, t = clip_outs(fx, dev)
    lay = [l.to(dev) for l in layers(fx)]
    (mav, wb), (pmav, pwb) = lay[0].tensors(dev), lay[1].tensors(dev)
    n = 2
    offs = torch.tensor(fx["clips"][:, 0], dtype=torch.float32, device=dev)
    fps = torch.tensor(fx["clips"][:, 1], dtype=torch.float32, device=dev)
    st = (ctypes.c_int64 * 3)(A * D, D, 1)
    bufs = dict(seg=guarded(n * A * 2, dev), score=guarded(n * K * A, dev), unknown=guarded(n * A, dev),
                flag=guarded(n * K * A, dev, torch.uint8))
    L.check(L.lib().otal_decode_clips_openmax(
        L.ptr(t['loc']), L.ptr(t['prop_loc']), L.ptr(t['priors']), L.ptr(t['conf']), L.ptr(t['prop_conf']), L.ptr(t['center']),
        L.ptr(offs), L.ptr(fps), L.ptr(t['conf_feat']), L.ptr(t['prop_conf_feat']) if refined else None, st, st if refined else None,
        L.ptr(mav), L.ptr(pmav), L.ptr(wb), L.ptr(pwb), L.ptr(bufs['seg'][1]), L.ptr(bufs['score'][1]), L.ptr(bufs['unknown'][1]),
        L.ptr(bufs['flag'][1]), n, A, K + 1, 1, D, 1, refined, 256.0, 0.01, L.stream()), "decode")
    for name, (buf, view) in bufs.items():
        check_guard(buf, view.numel(), "otal_decode_clips_openmax " + name)
    assert bool((bufs['flag'][1] <= 1).all())              # every flag byte was written (0 / 1, no sentinel left)


# ----------------------------------------------------------------------------- plumbing on the device
def test_get_matched_targets_on_the_device_equals_the_reference(fx, dev):
    from opental_amd.thumos14.test_openmax import get_matched_targets
    loc, targets = R.match_inputs(int(fx["seed_match"]))
    _, conf_t, _, prop_conf_t = get_matched_targets([torch.from_numpy(t) for t in targets], torch.from_numpy(loc).to(dev),
                                                    torch.from_numpy(R.priors()).to(dev), 256, 0.5)
    assert conf_t.is_cuda and np.array_equal(conf_t.cpu().numpy(), fx["match_conf_t"])
    assert np.array_equal(prop_conf_t.cpu().numpy(), fx["match_prop_conf_t"])


def closed_set_params(seed, head_seed):
    """tools/pin_closed_set.py closed_set_params (restated as in tests/test_closed_set_gpu.py)."""
    p = {k: v for k, v in arch.make_params(seed).items() if "actionness_head" not in k}
    rs = np.random.RandomState(head_seed)
    for head, k in (("conf_head", 3), ("prop_conf_head", 1)):
        key = f"coarse_pyramid_detection.{head}.conv1d"
        lim = np.sqrt(3.0 / max(1.0, (512 * k + (K + 1) * k) / 2.0))
        p[key + ".weight"] = rs.uniform(-lim, lim, size=(K + 1, 512, k)).astype(np.float32)
        p[key + ".bias"] = rs.uniform(-0.1, 0.1, size=(K + 1,)).astype(np.float32)
    return p


def test_model_features_match_the_reference(fx, dev):
    """conf_feat / prop_conf_feat of BDNet.forward(x, get_feat=True) against the reference's, within the bound
    tests/test_closed_set_gpu.py uses for the model forward (1e-4 of the largest magnitude)."""
    from opental_amd.common import ops
    from opental_amd.thumos14.BDNet import BDNet, DEFAULT_MODEL_CFG
    old = ops.CONV_PRECISION
    ops.CONV_PRECISION = 0
    try:
        net = BDNet(training=False, use_edl=False, cfg=dict(DEFAULT_MODEL_CFG, os_head=False))
        params = closed_set_params(int(fx["model_param_seed"]), int(fx["model_head_seed"]))
        net.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
        net = net.to(dev).eval()
        x = torch.from_numpy(arch.make_clip(int(fx["model_clip_seed"]), 1)).to(dev)
        with torch.no_grad():
            out = net(x, get_feat=True)
            plain = net(x)
        assert 'conf_feat' not in plain
        rel = lambda a, b: float(np.abs(np.asarray(a, np.float64) - b).max() / max(np.abs(b).max(), 1e-6))
        for k in ("conf_feat", "prop_conf_feat"):
            assert out[k].shape == (1, A, D)
            f = out[k].detach().reshape(-1)
            r_probe = rel(f[::max(1, f.numel() // 2048)].cpu().numpy(), fx[f"model_probe_{k}"])
            r_norm = rel(out[k][0].double().norm(dim=1).cpu().numpy(), fx[f"model_norm_{k}"])
            print(f"{k}: subsample rel err {r_probe:.3e}, per-anchor norm rel err {r_norm:.3e}")
            assert r_probe < 1e-4 and r_norm < 1e-4, k
    finally:
        ops.CONV_PRECISION = old


def test_driver_on_a_synthetic_dataset(tmp_path, fx):
    """python -m opental_amd.thumos14.test_openmax on a synthetic THUMOS14 layout rewritten to the Softmax baseline, random
    initialisation: writes the mav_dist files and the result JSON, reuses the files on a second run, and the detections of
    one video equal decode_clips_openmax + Soft-NMS on the same network outputs."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    from make_synthetic_thumos import CLASSES, make
    from opental_amd.common import ops
    from opental_amd.thumos14 import test as T, test_openmax as TO
    from opental_amd.thumos14.openmax import OpenMax
    old = ops.CONV_PRECISION
    src = make(str(tmp_path / "data"), videos=6, frames=400, size=100)
    # every known class must occur in the training split: hand the classes out in turn
    anno = str(tmp_path / "data" / "train_anno.csv")
    rows = open(anno).read().strip().split("\n")
    assert len(rows) - 1 >= len(CLASSES)
    for i in range(1, len(rows)):
        c = rows[i].split(",")
        c[2], c[1] = str(CLASSES[(i - 1) % len(CLASSES)][0]), CLASSES[(i - 1) % len(CLASSES)][1]
        rows[i] = ",".join(c)
    open(anno, "w").write("\n".join(rows) + "\n")
    cfg = yaml.load(open(src).read(), Loader=yaml.FullLoader)
    md, tr = cfg['model'], cfg['training']
    md.pop('os_head', None)
    tr.pop('act_config', None)
    md['use_edl'] = False
    tr['edl_loss'], tr['focal_loss'] = False, True
    cfg['testing']['output_json'] = 'openmax.json'
    path = str(tmp_path / "openmax.yaml")
    with open(path, "w") as f:
        yaml.dump(cfg, f)
    known = tmp_path / "known.txt"
    known.write_text(open(tmp_path / "data" / "classes.txt").read())
    argv = [path, '--open_set', '--split', '0', '--piou', '0', '--random_init']
    try:
        torch.manual_seed(0)
        out_file, metrics = TO.main(argv + ['--evaluate', str(tmp_path / "data" / "gt_open.json"), str(known)])
        mav_dir = os.path.join(cfg['testing']['output_path'], 'mav_dist')
        names = [n for _, n in CLASSES]
        assert sorted(os.listdir(mav_dir)) == sorted(n + ".npz" for n in names)
        data = np.load(os.path.join(mav_dir, names[0] + ".npz"))
        assert sorted(data.files) == ["dist", "dist_prop", "mav", "mav_prop"] and data["mav"].shape == (D,)
        assert data["dist"].ndim == 1 and data["dist"].size >= 2 and (data["dist"] >= 0).all()
        first = json.load(open(out_file))
        assert first["version"] == "THUMOS14" and len(first["results"]) == 2
        assert metrics is None or all(len(np.asarray(v)) == 5 for v in metrics.values())       # five tIoU thresholds
        props = [p for v in first["results"].values() for p in v]
        assert props and all(set(p) == {'label', 'score', 'segment', 'uncertainty', 'actionness'} for p in props)
        assert all(p['uncertainty'] == 0.0 and p['actionness'] == 0.0 and p['label'] in names for p in props)
        # second run: the files are there and are reused (their timestamps stay); same weights -> the same detections
        stamps = {n: os.path.getmtime(os.path.join(mav_dir, n)) for n in os.listdir(mav_dir)}
        torch.manual_seed(0)
        out_file2, _ = TO.main(argv)
        assert stamps == {n: os.path.getmtime(os.path.join(mav_dir, n)) for n in os.listdir(mav_dir)}
        assert json.load(open(out_file2))["results"] == first["results"]
        # one video by hand: the same network, its outputs decoded by decode_clips_openmax, then Soft-NMS
        from opental_amd.common import config as C
        from opental_amd.common.thumos_dataset import get_class_index_map, get_video_info
        from opental_amd.thumos14.BDNet import BDNet, model_cfg_from
        config = C.set_config(C.get_config([path, '--open_set', '--split', '0', '--piou', '0']))
        torch.manual_seed(0)
        dev = torch.device("cuda", 0)
        net = BDNet(in_channels=config['model']['in_channels'], training=False, use_edl=False, cfg=model_cfg_from(config)).to(dev).eval()
        _, idx_to_class = get_class_index_map(config['dataset']['class_info_path'])
        wm, wpm = TO.weibull_fitting(idx_to_class, mav_dir)
        lay = OpenMax(wm).to(dev), OpenMax(wpm).to(dev)
        ds, te = config['dataset']['testing'], config['testing']
        infos = get_video_info(ds['video_info_path'])
        # the same windows in the same batch as the driver's run (both videos in one forward pass)
        vids = [T.prepare_data(ds['video_data_path'], n, ds['crop_size'], dev) for n in infos]
        offs = [T.get_offsets(v.shape[1], ds['clip_length'], ds['clip_stride']) for v in vids]
        windows = [(v, o) for v in range(len(vids)) for o in offs[v]]
        with torch.no_grad():
            out = net(T.prepare_windows(vids, windows, ds['clip_length']), get_feat=True)
        fps = [float(infos[n]['sample_fps']) for v, n in enumerate(infos) for _ in offs[v]]
        dec = TO.decode_clips_openmax(out, [float(o) for _, o in windows], fps, lay[0], lay[1], ds['clip_length'], te['conf_thresh'])
        rows_, counts, _ = T.softnms_classes(dec, [0, len(offs[0]), len(windows)], te['top_k'], te['nms_sigma'])
        name = list(infos)[1]
        assert T.get_video_detections(rows_[1], counts[1], idx_to_class, te['top_k']) == first["results"][name]
    finally:
        ops.CONV_PRECISION = old
