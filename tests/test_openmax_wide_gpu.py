"""GPU: the OpenMax kernels for up to 256 classes (csrc/openmax_wide.hip), the ActivityNet model's get_feat outputs and the
driver opental_amd.anet.test_openmax, against tests/golden/openmax_wide.npz, which tools/pin_openmax_wide.py recorded from the
reference (its openmax.py over libMR, in float64) at K = 150.

Tolerances, as tests/test_openmax_gpu.py states them.  The yardstick is the reference in float64 -- the golden, or, for shapes
and cases the golden does not hold, the float64 restatement of tests/openmax_ref.py that tests/test_openmax_wide_cpu.py pins to
the golden to rtol 1e-9.  For probabilities, scores, `unknown` and distances the pin tool evaluated a plain float32 numpy
restatement (stable w-score form) and stored its largest absolute deviation from the reference as `tol_*`; every bound here
is 4x that figure: the factor covers the device's expf / log1pf / expm1f and another summation order over 512 terms.  No
kernel is compared with itself or with the package's torch code.  Each test prints its figures before it asserts."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch
import yaml

import openmax_ref as R
import openmax_wide_ref as W

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, D, A = W.K, W.D, W.A
GUARD = 4096
SENTINEL_F32 = 0x7F7FBEEF       # as tests/test_openmax_gpu.py: a finite pattern nobody writes by accident
SENTINEL_U8 = 0xA5


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "openmax_wide.npz"))


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def tol_probs(fx):
    return 4 * max(float(fx["tol_probs_r1"][0]), float(fx["tol_probs_r3"][0]))


def layer_of(mav, fits, rank=1):
    """anet.openmax.OpenMax over MAVs and float64 Weibull parameters dict(scale, shape, small) of (K,) arrays."""
    from opental_amd.anet.openmax import OpenMax, WeibullFit
    model = {f"class_{k + 1}": {'mean_vec': mav[k], 'model': [WeibullFit(fits['scale'][k], fits['shape'][k], fits['small'][k])]}
             for k in range(len(mav))}
    return OpenMax(model, rank=rank)


def layers(fx, dev, rank=1):
    cen, pcen = W.mavs(fx)
    return layer_of(cen, W.fits_of(fx, 0), rank).to(dev), layer_of(pcen, W.fits_of(fx, 1), rank).to(dev)


def worst(got, want):
    return float(np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64)).max())


def channel_major_view(t):
    """(B, A, D) or (N, D) values held channel-major, as the towers produce them: a permuted view, not a copy."""
    v = t.transpose(-1, -2).contiguous().transpose(-1, -2)
    assert not v.is_contiguous() and v.stride(-2) == 1 and torch.equal(v, t)
    return v


def up(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ----------------------------------------------------------------------------- 1. probabilities at K = 150
@pytest.mark.parametrize("rank", [1, 3])
def test_probabilities_match_the_reference(fx, dev, rank):
    feats, logits, _ = W.prob_rows(fx)
    layer = layers(fx, dev, rank)[0]
    bound = 4 * float(fx[f"tol_probs_r{rank}"][0])
    f, z = up(feats, dev), up(logits, dev)
    p = layer(z, f)
    assert p.shape == (64, K + 1) and p.dtype == torch.float32 and p.is_cuda
    part = layer(z[:37], f[:37])                            # a partial tile
    e_all, e_part = worst(p.cpu().numpy(), fx[f"probs_r{rank}"]), worst(part.cpu().numpy(), fx[f"probs_r{rank}"][:37])
    sums = float((p.double().sum(1) - 1).abs().max())
    print(f"probs rank {rank}: max abs err {e_all:.3e} (64 rows), {e_part:.3e} (37 rows), bound {bound:.3e}; |row sum - 1| {sums:.3e}")
    assert e_all <= bound and e_part <= bound
    assert sums < 1e-5
    assert torch.equal(part, p[:37]) and torch.equal(layer(z, f), p)        # the same bits per row, and in a second run


# ----------------------------------------------------------------------------- 2. the shape sweep
def sweep_case(k, d, n, seed):
    """Seeded inputs of any shape: clustered rows, logits favouring the row's class, Weibull parameters of the fixture's
    magnitude (shape ~ 2.5e5 on a translated tail, scale ~ 10000, small_score inside the rows' distances)."""
    rs = np.random.RandomState(seed)
    cen = R.class_centres(seed + 1, k, d)
    lab = rs.randint(0, k, n)
    feats = R.features_of(cen, lab, seed + 2)
    logits = R.logits_of(lab, seed + 3, k=k)
    own = W.eucos_own(cen[lab], feats)
    fits = dict(scale=10000.0 + rs.uniform(0.02, 0.2, k), shape=rs.uniform(1.5e5, 4e5, k),
                small=np.full(k, float(np.median(own))) * rs.uniform(0.8, 1.2, k))
    return cen, feats, logits, fits


# the edges: one slot, a second slot partly filled, the last lane of the last slot, a single row; R = K only for K <= 33
SWEEP = list(dict.fromkeys((k, d, n, r) for k in (1, 15, 16, 17, 33, 150, 256) for d in (16, 512) for n in (1, 37)
                           for r in (1, 3, k) if r == 1 or (r == 3 and k >= 3) or (r == k and k <= 33)))


@pytest.mark.parametrize("k,d,n,r", SWEEP)
def test_shape_sweep_matches_the_float64_restatement(dev, tol_probs, k, d, n, r):
    cen, feats, logits, fits = sweep_case(k, d, n, 1000 + 7 * k + d + n)
    want = R.openmax_probs(logits, feats, cen, fits, r)
    p = layer_of(cen, fits, r).to(dev)(up(logits, dev), up(feats, dev)).cpu().numpy()
    err = worst(p, want)
    print(f"K {k} D {d} N {n} R {r}: max abs err {err:.3e}, bound {tol_probs:.3e}; P(unknown) up to {want[:, 0].max():.3g}")
    assert p.shape == (n, k + 1) and err <= tol_probs


# ----------------------------------------------------------------------------- 3. K = 15 on the wide kernel
@pytest.mark.parametrize("rank", [1, 3])
def test_fifteen_classes_answer_to_the_narrow_fixture(golden_dir, dev, rank):
    """tests/golden/openmax.npz (tools/pin_openmax.py, K = 15) through the WIDE kernel, within that fixture's own bound."""
    nfx = np.load(os.path.join(golden_dir, "openmax.npz"))
    lab = nfx["rows_labels"].astype(np.int64)
    seed = int(nfx["seed_rows"])
    feats = R.features_of(R.class_centres(int(nfx["seed_centres"])), lab, seed + 1)
    logits = R.logits_of(lab, seed + 2)
    par = nfx["fit_params"][:R.K]
    layer = layer_of(nfx["mav"], dict(scale=par[:, 0], shape=par[:, 1], small=par[:, 2]), rank).to(dev)
    p = layer(up(logits, dev), up(feats, dev)).cpu().numpy()
    bound = 4 * float(nfx[f"tol_probs_r{rank}"][0])
    err = worst(p, nfx[f"probs_r{rank}"])
    print(f"K = 15 fixture on the wide kernel, rank {rank}: max abs err {err:.3e}, bound {bound:.3e}")
    assert p.shape == (256, R.K + 1) and err <= bound


# ----------------------------------------------------------------------------- 4. ties
@pytest.mark.parametrize("pair", [(3, 4), (3, 19), (0, 149)])
@pytest.mark.parametrize("rank", [1, 2])
def test_equal_logits_rank_the_higher_index_first(fx, dev, tol_probs, pair, rank):
    """Exactly equal float32 logits: the higher index takes the larger alpha, which is what `argsort()[::-1]` gives wherever
    numpy's sort keeps equal keys in order (rows of 15: tests/test_openmax_gpu.py; at 150 entries numpy's default sort is not
    stable and orders a tie either way).  The golden holds no ties, so the float64 restatement is the yardstick; it is handed
    the kernel's float32 logits with the higher index raised by ONE float64 ulp (1e-16 relative, nothing against the bound),
    which makes its argsort()[::-1] rank the pair as stated.  (3, 4): adjacent lanes; (3, 19): one lane, two slots; (0, 149):
    the first and the last class."""
    feats, logits, _ = W.prob_rows(fx, 32)
    logits = logits.copy()
    lo, hi = pair
    logits[:, lo] = logits[:, hi] = logits.max(1) + np.float32(1.0)
    assert (logits[:, lo] == logits[:, hi]).all()
    z64 = logits.astype(np.float64)
    z64[:, hi] = np.nextafter(z64[:, hi], np.inf)
    assert (np.argsort(z64, 1)[:, -1] == hi).all() and (np.argsort(z64, 1)[:, -2] == lo).all()
    cen = W.mavs(fx)[0]
    want = R.openmax_probs(z64, feats, cen, W.fits_of(fx, 0), rank)
    p = layers(fx, dev, rank)[0](up(logits, dev), up(feats, dev)).cpu().numpy()
    err = worst(p, want)
    gap = float(np.abs(want[:, 1 + lo] - want[:, 1 + hi]).max())
    print(f"tie {pair} rank {rank}: max abs err {err:.3e}, bound {tol_probs:.3e}; the tied classes differ by up to {gap:.3e}")
    assert err <= tol_probs
    assert gap > 1e-3                                       # the higher index took the larger alpha: the two come out differently
    # the other order of the tie is a different answer, farther away than the bound
    swapped = want.copy()
    swapped[:, [1 + lo, 1 + hi]] = want[:, [1 + hi, 1 + lo]]
    assert worst(p, swapped) > 100 * tol_probs


# ----------------------------------------------------------------------------- 5. layouts, 6. labelled distances
def test_both_feature_layouts_give_the_same_bits(fx, dev):
    from opental_amd.anet.openmax import compute_eucos_dist
    feats, logits, lab = W.prob_rows(fx)
    layer = layers(fx, dev, 3)[0]
    f, z, l = up(feats, dev), up(logits, dev), up(lab.astype(np.int32), dev)
    fv = channel_major_view(f)
    assert torch.equal(layer(z, fv), layer(z, f))
    mav = layer.mav
    assert torch.equal(compute_eucos_dist(mav, fv, l), compute_eucos_dist(mav, f, l))
    three = f.reshape(4, 16, D)                             # (B, A, D) and its channel-major view, row by row the same
    assert torch.equal(compute_eucos_dist(mav, channel_major_view(three), l), compute_eucos_dist(mav, f, l))
    wide = torch.cat([torch.full((64, 1), 9.0, device=dev), z], 1)         # a `conf[:, 1:]` view: ldl = K + 1
    assert torch.equal(layer(wide[:, 1:], f), layer(z, f))


@pytest.mark.parametrize("tag", ["", "_prop"])
def test_labelled_distances_match_float64(fx, dev, tag):
    from opental_amd.anet.openmax import compute_eucos_dist
    cen = W.mavs(fx)[1 if tag else 0]
    feats, labels = W.stat_rows(cen, int(fx["seed_prop_stat" if tag else "seed_stat"]))
    feats, labels = feats[:1111], labels[:1111]             # every class, several tiles, a partial last one
    want = W.eucos_own(cen[labels], feats)
    bound = 4 * float(fx["tol_dist" + tag][0])
    mav, f = up(cen, dev), up(feats, dev)
    got = compute_eucos_dist(mav, f, up(labels, dev))
    err = worst(got.cpu().numpy(), want)
    print(f"labelled dist{tag}: {len(labels)} rows, max abs err {err:.3e}, bound {bound:.3e}")
    assert got.shape == (1111,) and err <= bound
    lab = up(labels.astype(np.int32), dev).clone()
    lab[5], lab[17], lab[1110] = -1, K, K + 7
    marked = compute_eucos_dist(mav, f, lab).cpu().numpy()
    assert marked[5] == -1 and marked[17] == -1 and marked[1110] == -1
    keep = np.setdiff1d(np.arange(1111), [5, 17, 1110])
    assert np.array_equal(marked[keep], got.cpu().numpy()[keep])


# ----------------------------------------------------------------------------- 7. decode
def clip_outs(fx, dev):
    cen, pcen = W.mavs(fx)
    outs = W.clip_outputs(int(fx["seed_decode"]), cen, pcen)
    t = {k: up(v, dev) for k, v in outs.items()}
    t['priors'] = up(W.priors(), dev)
    return outs, t


@pytest.fixture(scope="module")
def decode_refs(fx):
    """float64 scores (n, K + 1, A) of the decode case, as shipped and with the refined feature (computed once)."""
    cen, pcen = W.mavs(fx)
    outs = W.clip_outputs(int(fx["seed_decode"]), cen, pcen)
    args = (cen, W.fits_of(fx, 0), pcen, W.fits_of(fx, 1))
    return W.decode(outs, *args), W.decode(outs, *args, refined_feature=True)


@pytest.mark.parametrize("refined", [0, 1])
def test_decode_matches_the_reference(fx, dev, decode_refs, refined):
    from opental_amd.anet.test_openmax import decode_clips_openmax
    _, t = clip_outs(fx, dev)
    lay = layers(fx, dev)
    thr, clip_length = float(fx["decode_params"][0]), float(fx["decode_params"][1])
    fps = fx["clips"][:, 1].tolist()
    dec = decode_clips_openmax(t, fps, lay[0], lay[1], clip_length, thr, refined_feature=bool(refined))
    assert dec['unct'] is None and dec['actn'] is None and dec['score'].shape == (2, K, A) and dec['flag'].dtype == torch.uint8
    b_score, b_unk = 4 * float(fx["tol_score"][0]), 4 * float(fx["tol_unknown"][0])
    score, ref = dec['score'].cpu().numpy(), decode_refs[refined]
    e_score, e_unk = worst(score, ref[:, 1:]), worst(dec['unknown'].cpu().numpy(), ref[:, 0])
    close = np.abs(ref[:, 1:] - thr) <= b_score
    print(f"decode refined {refined}: score max abs err {e_score:.3e} (bound {b_score:.3e}), unknown {e_unk:.3e} (bound "
          f"{b_unk:.3e}); {close.sum()} of {close.size} cells ({100.0 * close.mean():.3f} %) within the bound of the threshold")
    assert e_score <= b_score and e_unk <= b_unk
    flag = dec['flag'].cpu().numpy()
    if not refined:                                         # the golden itself: stored anchors, and the mask of every cell
        anchors = fx["decode_anchors"].astype(np.int64)
        e_gold = worst(score[:, :, anchors], fx["decode_score"][:, 1:])
        print(f"  against the golden's {len(anchors)} anchors: {e_gold:.3e}")
        assert e_gold <= b_score
        assert np.array_equal(flag[~close], fx["decode_mask"][:, 1:][~close])
    np.testing.assert_allclose(dec['seg'].cpu().numpy(), fx["decode_seg"], rtol=1e-6, atol=1e-5)
    assert close.sum() <= 0.01 * close.size
    assert np.array_equal(flag[~close].astype(bool), (ref[:, 1:] > thr)[~close])
    assert np.array_equal(flag.astype(bool), score > thr) and set(np.unique(flag).tolist()) <= {0, 1}
    # deterministic, and the same bits from channel-major feature views
    again = decode_clips_openmax(t, fps, lay[0], lay[1], clip_length, thr, refined_feature=bool(refined))
    t2 = dict(t, conf_feat=channel_major_view(t['conf_feat']), prop_conf_feat=channel_major_view(t['prop_conf_feat']))
    strided = decode_clips_openmax(t2, fps, lay[0], lay[1], clip_length, thr, refined_feature=bool(refined))
    for k in ('seg', 'score', 'unknown', 'flag'):
        assert torch.equal(again[k], dec[k]) and torch.equal(strided[k], dec[k]), k


def test_refined_feature_switch_is_live(fx, dev, decode_refs):
    from opental_amd.anet.test_openmax import decode_clips_openmax
    _, t = clip_outs(fx, dev)
    lay = layers(fx, dev)
    args = (fx["clips"][:, 1].tolist(), lay[0], lay[1], float(fx["decode_params"][1]), float(fx["decode_params"][0]))
    a = decode_clips_openmax(t, *args, refined_feature=False)['score'].cpu().numpy()
    b = decode_clips_openmax(t, *args, refined_feature=True)['score'].cpu().numpy()
    moved, want = worst(a, b), worst(decode_refs[0][:, 1:], decode_refs[1][:, 1:])
    print(f"refined_feature moves a score by up to {moved:.3e} (float64 restatement: {want:.3e})")
    assert moved > 1e-2 and abs(moved - want) <= 8 * float(fx["tol_score"][0])


# ----------------------------------------------------------------------------- 8. guards
def guarded(n, dev, dtype=torch.float32):
    """A sentinel-filled buffer with GUARD elements on either side of an n-element output view."""
    if dtype == torch.uint8:
        buf = torch.full((n + 2 * GUARD,), SENTINEL_U8, dtype=torch.uint8, device=dev)
    else:
        buf = torch.full((n + 2 * GUARD,), SENTINEL_F32, dtype=torch.int32, device=dev).view(dtype)
    return buf, buf[GUARD:GUARD + n]


def check_guard(buf, n, name):
    raw = buf.view(torch.int32) if buf.dtype != torch.uint8 else buf
    s = SENTINEL_U8 if buf.dtype == torch.uint8 else SENTINEL_F32
    assert bool((raw[:GUARD] == s).all()) and bool((raw[GUARD + n:] == s).all()), f"{name}: wrote outside its output"
    if buf.dtype != torch.uint8:
        assert not bool((raw[GUARD:GUARD + n] == s).any()), f"{name}: left part of its output unwritten"


@pytest.mark.parametrize("n_rows,k", [(37, 150), (256, 17)])
def test_launches_write_their_whole_output_and_nothing_else(dev, n_rows, k):
    from opental_amd import _lib as L
    cen, feats, logits, fits = sweep_case(k, D, n_rows, 77)
    layer = layer_of(cen, fits).to(dev)
    f, z = up(feats, dev), up(logits, dev)
    lab = up(np.random.RandomState(5).randint(-1, k + 1, n_rows).astype(np.int32), dev)    # some labels outside [0, K)
    mav, wb = layer.tensors(dev)
    lib = L.lib()
    view = (n_rows, 0, D, 1)
    buf, out = guarded(n_rows, dev)
    L.check(lib.otal_openmax_dist_wide(L.ptr(f), n_rows, *view, L.ptr(mav), k, D, L.ptr(lab), L.ptr(out), L.stream()), "dist")
    check_guard(buf, n_rows, "otal_openmax_dist_wide")
    buf, out = guarded(n_rows * (k + 1), dev)
    L.check(lib.otal_openmax_probs_wide(L.ptr(z), k, L.ptr(f), n_rows, *view, L.ptr(mav), L.ptr(wb), k, D, 1, L.ptr(out),
                                        L.stream()), "probs")
    check_guard(buf, n_rows * (k + 1), "otal_openmax_probs_wide")


@pytest.mark.parametrize("refined", [0, 1])
def test_decode_launch_writes_its_whole_output_and_nothing_else(fx, dev, refined):
    from opental_amd import _lib as L
    _, t = clip_outs(fx, dev)
    lay = layers(fx, dev)
    (mav, wb), (pmav, pwb) = lay[0].tensors(dev), lay[1].tensors(dev)
    n = 2
    offs = torch.zeros(n, dtype=torch.float32, device=dev)
    fps = torch.tensor(fx["clips"][:, 1], dtype=torch.float32, device=dev)
    pri = t['priors'][:, 0].contiguous()
    st = (ctypes.c_int64 * 3)(A * D, D, 1)
    bufs = dict(seg=guarded(n * A * 2, dev), score=guarded(n * K * A, dev), unknown=guarded(n * A, dev),
                flag=guarded(n * K * A, dev, torch.uint8))
    L.check(L.lib().otal_decode_clips_openmax_wide(
        L.ptr(t['loc']), L.ptr(t['prop_loc']), L.ptr(pri), L.ptr(t['conf']), L.ptr(t['prop_conf']), L.ptr(t['center']),
        L.ptr(offs), L.ptr(fps), L.ptr(t['conf_feat']), L.ptr(t['prop_conf_feat']) if refined else None, st, st if refined else None,
        L.ptr(mav), L.ptr(pmav), L.ptr(wb), L.ptr(pwb), L.ptr(bufs['seg'][1]), L.ptr(bufs['score'][1]), L.ptr(bufs['unknown'][1]),
        L.ptr(bufs['flag'][1]), n, A, K + 1, 1, D, 1, refined, 768.0, 0.001, L.stream()), "decode")
    for name, (buf, view) in bufs.items():
        check_guard(buf, view.numel(), "otal_decode_clips_openmax_wide " + name)
    assert bool((bufs['flag'][1] <= 1).all())              # every flag byte was written (0 / 1, no sentinel left)


# ----------------------------------------------------------------------------- 9. the model
def test_model_returns_the_head_inputs_with_get_feat(dev):
    """anet.BDNet in eval mode: get_feat adds conf_feat / prop_conf_feat (1, 189, 512) and changes nothing else; they ARE the
    head inputs: conf = conf_head(conf_feat) (k = 3, SAME padding inside each pyramid level) and prop_conf =
    prop_conf_head(prop_conf_feat) (k = 1), by a plain float64 conv1d, within rel 1e-4 (the project's fp32 parity bound)."""
    import torch.nn.functional as F
    from oracle import arch
    from opental_amd.common import ops
    from opental_amd.anet.BDNet import BDNet, DEFAULT_MODEL_CFG
    old = ops.CONV_PRECISION
    ops.CONV_PRECISION = 0
    try:
        torch.manual_seed(7)
        net = BDNet(training=False, use_edl=False, cfg=dict(DEFAULT_MODEL_CFG, os_head=False)).to(dev).eval()
        x = torch.from_numpy(arch.make_clip(11, 1, frames=768)).to(dev)
        with torch.no_grad():
            out = net(x, get_feat=True)
            plain = net(x)
        assert 'conf_feat' not in plain and 'prop_conf_feat' not in plain
        assert set(out) == set(plain) | {'conf_feat', 'prop_conf_feat'}
        for k, v in plain.items():
            assert (v is None and out[k] is None) or torch.equal(out[k], v), k
        cpd = net.coarse_pyramid_detection
        lev = np.cumsum((0,) + W.LEVELS)
        for feat_key, conf_key, head in (("conf_feat", "conf", cpd.conf_head), ("prop_conf_feat", "prop_conf", cpd.prop_conf_head)):
            assert out[feat_key].shape == (1, A, D) and out[conf_key].shape == (1, A, 151)
            w, b = head.conv1d.weight.detach().double().cpu(), head.conv1d.bias.detach().double().cpu()
            xin = out[feat_key].double().cpu().permute(0, 2, 1)
            want = torch.cat([F.conv1d(xin[:, :, a:e], w, b, padding=w.shape[-1] // 2) for a, e in zip(lev[:-1], lev[1:])], 2)
            want = want.permute(0, 2, 1)
            rel = float((out[conf_key].double().cpu() - want).abs().max() / want.abs().max())
            print(f"{conf_key} = head({feat_key}): rel err {rel:.3e}; |{feat_key}| up to {float(out[feat_key].abs().max()):.3g}")
            assert float(want.abs().max()) > 0 and rel < 1e-4, conf_key
    finally:
        ops.CONV_PRECISION = old


# ----------------------------------------------------------------------------- 10. the driver
CLASSES = ["Long jump", "Playing violin", "Mowing the lawn"]


def _anet_openmax_set(root, size=100, seed=3):
    """A tiny ActivityNet-layout set (after tests/test_drivers_gpu.py::_anet_validation_set): two training videos per class
    with annotations in frames, two validation videos (one shorter than a clip), the class list and the Softmax baseline's yaml."""
    rs = np.random.RandomState(seed)
    vdir = os.path.join(root, "npy")
    os.makedirs(vdir, exist_ok=True)
    info = {}

    def video(name, frames):
        np.save(os.path.join(vdir, name + ".npy"), rs.randint(0, 256, (frames, size, size, 3)).astype(np.uint8))
    for v in range(6):
        name, frames = f"v_train{v:04d}", 768 if v % 2 == 0 else 600
        video(name, frames)
        start = 100 + 40 * v                                # a 120-frame action: levels 2 and 3 admit it (bounds 30-120, 60-240)
        info[name] = {"subset": "training", "fps": 10.0, "frame_num": frames, "duration": frames / 10.0,
                      "annotations": [{"label": CLASSES[v % 3], "label_id": v % 3 + 1, "start_frame": start, "end_frame": start + 120,
                                       "segment": [start / 10.0, (start + 120) / 10.0]}]}
    for v in range(2):
        name, frames = f"v_val{v:04d}", 768 if v == 0 else 420
        video(name, frames)
        info[name] = {"subset": "validation", "fps": 5.0 + v, "frame_num": frames, "duration": frames / (5.0 + v),
                      "annotations": [{"label": CLASSES[v], "label_id": v + 1, "start_frame": 50, "end_frame": 200,
                                       "segment": [50 / (5.0 + v), 200 / (5.0 + v)]}]}
    info_path = os.path.join(root, "video_info.json")
    with open(info_path, "w") as f:
        json.dump(info, f)
    with open(os.path.join(REPO, "configs", "anet_opental.yaml")) as f:
        cfg = yaml.load(f.read(), Loader=yaml.FullLoader)
    for part in ("training", "testing"):
        cfg["dataset"][part].update(video_mp4_path=vdir, video_info_path=info_path)
    cfg["dataset"]["num_classes"] = len(CLASSES) + 1
    cfg["dataset"]["class_info_path"] = os.path.join(root, "action_known.txt")
    with open(cfg["dataset"]["class_info_path"], "w") as f:
        f.write("".join(c + "\n" for c in CLASSES))
    md, tr = cfg["model"], cfg["training"]              # the Softmax baseline: closed set, focal loss, no EDL
    md.pop("os_head", None)
    md["use_edl"] = False
    tr["edl_loss"], tr["focal_loss"] = False, True
    tr["checkpoint_path"] = os.path.join(root, "ckpt")
    cfg["testing"].update(checkpoint_path=os.path.join(root, "ckpt", "checkpoint-latest.ckpt"),
                          output_path=os.path.join(root, "output"), output_json="openmax_results.json", conf_thresh=0.001)
    path = os.path.join(root, "anet_softmax.yaml")
    with open(path, "w") as f:
        yaml.dump(cfg, f)
    return path, info, cfg


def test_driver_on_a_synthetic_activitynet_set(tmp_path, monkeypatch):
    """python -m opental_amd.anet.test_openmax with random weights: statistics pass -> six mav_dist files, fits, test pass ->
    the result file under <output_path>/openmax; a second call re-uses the files; a multi-rank call without them raises.
    (--piou 0, the config's default: with random weights the coarse segments are a few frames long, and a tIoU bar would
    leave each video its single best anchor.)"""
    from opental_amd.common import ops
    from opental_amd.anet import test_openmax as ATO
    old = ops.CONV_PRECISION
    path, info, cfg = _anet_openmax_set(str(tmp_path))
    argv = [path, '--open_set', '--split', '0', '--random_init']
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    try:
        torch.manual_seed(0)
        out_file = ATO.main(argv)
        out_dir = os.path.join(cfg["testing"]["output_path"], "openmax")
        assert out_file == os.path.join(out_dir, "openmax_results.json") and os.path.exists(out_file)
        assert not os.path.exists(os.path.join(cfg["testing"]["output_path"], "openmax_results.json"))
        mav_dir = os.path.join(out_dir, "mav_dist")
        assert sorted(os.listdir(mav_dir)) == sorted(c + ".npz" for c in CLASSES)
        counts = {}
        for c in CLASSES:
            data = np.load(os.path.join(mav_dir, c + ".npz"))
            assert sorted(data.files) == ["dist", "dist_prop", "mav", "mav_prop"]
            assert data["mav"].shape == (D,) and data["mav_prop"].shape == (D,)
            assert data["dist"].ndim == 1 and (data["dist"] >= 0).all() and (data["dist_prop"] >= 0).all()
            counts[c] = (int(data["dist"].size), int(data["dist_prop"].size))
        print(f"positives per class (coarse, refined): {counts}")
        assert all(n >= 2 and m >= 2 for n, m in counts.values())          # two videos per class, each with its action
        res = json.load(open(out_file))
        assert res["version"] == "ActivityNet-v1.3" and res["external_data"] == {}
        assert sorted(res["results"]) == ["val0000", "val0001"]
        total = 0
        for name, props in res["results"].items():
            duration = info["v_" + name]["duration"]
            total += len(props)
            for p in props:
                assert set(p) == {'label', 'score', 'segment', 'uncertainty', 'actionness'}
                assert p['label'] in CLASSES and 0.0 <= p['segment'][0] < p['segment'][1] <= duration
                assert 0.0 < p['score'] <= 1.0 and p['uncertainty'] == 0.0 and p['actionness'] == 0.0
        print(f"{total} detections in 2 validation videos")
        assert total > 0
        # a second call finds the mav_dist files and leaves them alone
        stamps = {n: os.path.getmtime(os.path.join(mav_dir, n)) for n in os.listdir(mav_dir)}
        torch.manual_seed(0)
        assert ATO.main(argv) == out_file
        assert stamps == {n: os.path.getmtime(os.path.join(mav_dir, n)) for n in os.listdir(mav_dir)}
        assert json.load(open(out_file))["results"] == res["results"]        # the same weights: the same detections
        # several ranks and no files: the statistics pass is to be run once, in one process
        for n in os.listdir(mav_dir):
            os.remove(os.path.join(mav_dir, n))
        monkeypatch.setenv("WORLD_SIZE", "2")
        with pytest.raises(RuntimeError, match="one process"):
            ATO.main(argv)
        assert os.listdir(mav_dir) == []
        # an open-set head is refused
        cfg["model"]["os_head"] = True
        bad = str(tmp_path / "bad.yaml")
        with open(bad, "w") as f:
            yaml.dump(cfg, f)
        monkeypatch.delenv("WORLD_SIZE")
        with pytest.raises(NotImplementedError):
            ATO.main([bad, '--open_set', '--split', '0', '--random_init'])
    finally:
        ops.CONV_PRECISION = old
