"""GPU: training the optical-flow stream (2-channel clips as zero-padded 3-plane batches).

  1. otal_prepare_clips_ch (csrc/input.hip) against numpy, bit for bit, with NaN-filled outputs and a NaN guard band;
  2. ClipStager(channels=2) on tests/golden/flow_dataset.npz: planes 0 and 1 are the reference's clips and ssl clips
     (AFSD/common/thumos_dataset.py:239-275, run by tools/pin_flow_dataset.py), plane 2 is zero;
  3. Conv3d_1a on a zero-plane batch (2-slice weight extended by a zero slice, the Conv3d_1a kernels) against today's generic
     chain on the 2-plane clip, forward and weight gradient, at the model's first-layer geometry;
  4. the trainer at b = 1 on a random-initialised BDNet(in_channels=2): arena gradients equal plain autograd; replayed lane
     graphs equal eager steps bit for bit;
  5. the trainer's checkpoint loads into the test drivers' flow network and runs a two-stream detect_batch;
  6. the training driver on a yaml with `model.in_channels: 2`: trains, resumes bit for bit, refuses rgb frames."""
import ctypes
import os

import numpy as np
import pytest
import torch

import flow_cases as F

pytestmark = pytest.mark.gpu
GUARD = 1024        # floats of NaN behind every output


# ----------------------------------------------------------------------------- 1. the kernel against numpy
def _norm(px):
    return (px.astype(np.float32) / np.float32(255.0)) * np.float32(2.0) - np.float32(1.0)


def _reference(frames, recs, fmap, cs, co, T, Hs, Ws, Ho, Wo):
    """(out, out_ssl) as otal_prepare_clips_ch defines them; `frames` is the flat uint8 buffer."""
    B = len(recs)
    outs = [np.full((B, co, T, Ho, Wo), np.nan, np.float32) for _ in range(2)]
    for b, (frame0, valid_t, ci, cj, flip) in enumerate(recs):
        src = frames[frame0: frame0 + valid_t * Hs * Ws * cs].reshape(valid_t, Hs, Ws, cs)
        pad = (np.float32(127.5 if flip & 2 else 0.0) / np.float32(255.0)) * np.float32(2.0) - np.float32(1.0)
        for which, out in enumerate(outs):
            for t in range(T):
                ts = int(fmap[b, t]) if which == 1 else t
                if 0 <= ts < valid_t:
                    crop = src[ts, ci: ci + Ho, cj: cj + Wo]
                    if flip & 1:
                        crop = crop[:, ::-1]
                    out[b, :cs, t] = _norm(crop).transpose(2, 0, 1)
                else:
                    out[b, :cs, t] = pad
            out[b, cs:] = np.float32(0.0)
    return outs


def _launch(entry, frames, recs, fmap, cs, co, T, Hs, Ws, Ho, Wo, want_out=True, want_ssl=True, misalign=0):
    """Run one entry on NaN-filled outputs with a NaN guard band behind them; returns numpy (out, out_ssl) or None each."""
    from opental_amd import _lib as L
    from opental_amd.common.input_pipeline import _PARAM_DTYPE
    dev = torch.device("cuda", 0)
    B = len(recs)
    n = B * co * T * Ho * Wo
    rec = np.zeros(B, _PARAM_DTYPE)
    for b, r in enumerate(recs):
        rec[b] = r
    d_frames = torch.from_numpy(frames).to(dev)
    d_params = torch.from_numpy(rec.view(np.uint8).copy()).to(dev)
    d_map = torch.from_numpy(np.ascontiguousarray(fmap, np.int32)).to(dev)
    bufs = [torch.full((misalign + n + GUARD,), float("nan"), dtype=torch.float32, device=dev) if want else None
            for want in (want_out, want_ssl)]
    ptrs = [None if b_ is None else ctypes.c_void_p(b_.data_ptr() + 4 * misalign) for b_ in bufs]
    lib = L.lib()
    if entry == "ch":
        rc = lib.otal_prepare_clips_ch(L.ptr(d_frames), L.ptr(d_params), L.ptr(d_map) if want_ssl else None, ptrs[0], ptrs[1],
                                       B, cs, co, T, Hs, Ws, Ho, Wo, L.stream())
    else:
        assert cs == co == 3
        rc = lib.otal_prepare_clips_map(L.ptr(d_frames), L.ptr(d_params), L.ptr(d_map) if want_ssl else None, ptrs[0], ptrs[1],
                                        B, T, Hs, Ws, Ho, Wo, L.stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    res = []
    for b_ in bufs:
        if b_ is None:
            res.append(None)
            continue
        h = b_.cpu().numpy()
        assert np.isnan(h[:misalign]).all() and np.isnan(h[misalign + n:]).all(), "wrote outside the output"
        res.append(h[misalign: misalign + n].reshape(B, co, T, Ho, Wo))
    return res


def _case(B, T, Hs, Ws, Ho, Wo, cs, flips, valid=(5, 2, 0), seed=0):
    """Frames, records and a frame map: a different frame0 per clip (the first one ODD: no 16-bit alignment of its pixels),
    valid_t cycling through `valid`, crops at (0,0), the far corner and an interior point, the given flip bits; a frame map
    with a negative entry and one >= valid_t in every clip."""
    rs = np.random.RandomState(seed)
    per = T * Hs * Ws * cs
    frames = rs.randint(0, 256, 7 + B * (per + 3 * cs)).astype(np.uint8)
    corners = [(0, 0), (Hs - Ho, Ws - Wo), ((Hs - Ho) // 2, (Ws - Wo + 1) // 2)]
    recs, pos = [], 7
    for b in range(B):
        vt = min(valid[b % len(valid)], T)
        ci, cj = corners[b % 3]
        recs.append((pos, vt, ci, cj, flips[b % len(flips)]))
        pos += per + 3 * cs - (b % 2)           # odd and even starts
    fmap = np.stack([rs.permutation(T) for _ in range(B)]).astype(np.int32)
    fmap[:, 1] = -1
    fmap[:, T - 1] = [r[1] for r in recs]       # == valid_t: the first frame past the clip's frames
    fmap[:, 0] = 0
    return frames, recs, fmap


def _check(got, want, cs, co):
    for g, w in zip(got, want):
        if g is None:
            continue
        assert not np.isnan(g).any(), "an element was never written"
        assert np.array_equal(g, w)
        if co > cs:
            assert not np.signbit(g[:, cs:]).any() and (g[:, cs:] == 0).all()      # +0.0, the sign bit clear


@pytest.mark.parametrize("planes", [(2, 3), (2, 2), (3, 3)])
def test_prepare_clips_ch_equals_numpy_bit_for_bit(planes):
    cs, co = planes
    T, Hs, Ws, Ho, Wo = 5, 9, 11, 6, 7
    for flips in ((0, 1, 2), (3, 2, 1)):
        frames, recs, fmap = _case(3, T, Hs, Ws, Ho, Wo, cs, flips)
        assert [r[1] for r in recs] == [5, 2, 0] and [r[2:4] for r in recs] == [(0, 0), (3, 4), (1, 2)] and recs[0][0] % 2
        want = _reference(frames, recs, fmap, cs, co, T, Hs, Ws, Ho, Wo)
        got = _launch("ch", frames, recs, fmap, cs, co, T, Hs, Ws, Ho, Wo)
        _check(got, want, cs, co)
        if planes == (3, 3):
            older = _launch("map", frames, recs, fmap, 3, 3, T, Hs, Ws, Ho, Wo)
            assert np.array_equal(older[0], got[0]) and np.array_equal(older[1], got[1])


@pytest.mark.parametrize("planes", [(2, 3), (3, 3)])
@pytest.mark.parametrize("misalign", [0, 1])
def test_prepare_clips_ch_four_pixel_groups_and_a_volume_that_is_no_multiple_of_256(planes, misalign):
    """Wo % 4 == 0: the 16-byte-store form of the kernel (misalign 0), or -- an output that is not 16-byte aligned -- the
    one-pixel form on the same shape; T * Ho * Wo = 360."""
    cs, co = planes
    T, Hs, Ws, Ho, Wo = 5, 9, 14, 6, 12
    frames, recs, fmap = _case(3, T, Hs, Ws, Ho, Wo, cs, (1, 2, 0))
    want = _reference(frames, recs, fmap, cs, co, T, Hs, Ws, Ho, Wo)
    _check(_launch("ch", frames, recs, fmap, cs, co, T, Hs, Ws, Ho, Wo, misalign=misalign), want, cs, co)


def test_prepare_clips_ch_with_only_the_ssl_output_and_with_only_the_plain_output():
    T, Hs, Ws, Ho, Wo = 5, 9, 11, 6, 7
    frames, recs, fmap = _case(3, T, Hs, Ws, Ho, Wo, 2, (1, 0, 3))
    want = _reference(frames, recs, fmap, 2, 3, T, Hs, Ws, Ho, Wo)
    got = _launch("ch", frames, recs, fmap, 2, 3, T, Hs, Ws, Ho, Wo, want_out=False)
    assert got[0] is None
    _check(got, want, 2, 3)
    got = _launch("ch", frames, recs, fmap, 2, 3, T, Hs, Ws, Ho, Wo, want_ssl=False)
    assert got[1] is None
    _check(got, want, 2, 3)


@pytest.mark.parametrize("wo", [19, 40])
def test_prepare_clips_ch_grid_stride(wo):
    """600 clips leave three workgroups per clip (the grid is capped near 2048 workgroups): a clip of more than 768 pixels
    (Wo 19, one-pixel form) or pixel groups (Wo 40, four-pixel form) takes the grid-stride loop."""
    T, Hs, Ho = (5, 10, 9) if wo == 19 else (8, 11, 10)
    Ws = wo + 2
    assert T * Ho * wo // (4 if wo % 4 == 0 else 1) > 768
    frames, recs, fmap = _case(600, T, Hs, Ws, Ho, wo, 2, (0, 1, 2, 3), valid=(T, 2, 0, T - 1))
    want = _reference(frames, recs, fmap, 2, 3, T, Hs, Ws, Ho, wo)
    _check(_launch("ch", frames, recs, fmap, 2, 3, T, Hs, Ws, Ho, wo), want, 2, 3)


# ----------------------------------------------------------------------------- 2. the dataset fixture through ClipStager
def test_clip_stager_reproduces_the_reference_flow_clips(golden_dir):
    from opental_amd.common import thumos_dataset as D
    from opental_amd.common.input_pipeline import is_zero_plane
    fx = np.load(os.path.join(golden_dir, "flow_dataset.npz"))
    infos, annos, videos = F.dataset_tables(fx["frames"])
    data = {n: torch.from_numpy(v).pin_memory() for n, v in videos.items()}
    ds = D.THUMOS_Dataset(data, infos, annos, clip_length=F.CLIP, crop_size=F.CROP, stride=F.STRIDE)
    samples = []
    for k, (idx, _) in enumerate(fx["picks"]):
        i, j, flip, offset, flag, valid = (int(v) for v in fx[f"decision_{k}"])
        fm = fx[f"map_{k}"]
        samples.append({'video': ds.data_dict[ds.training_list[int(idx)]['video_name']], 'offset': offset,
                        'crop': (i, j, bool(flip)), 'frame_map': fm if fm.size else None, 'flag': bool(flag)})
    H, W = fx["frames"].shape[1:3]
    stager = D.ClipStager(len(samples), F.CLIP, H, W, F.CROP, channels=2)
    assert stager.frame_bytes == H * W * 2 and stager.stage[0].numel() == len(samples) * F.CLIP * H * W * 2
    with pytest.raises(RuntimeError):
        stager.submit([dict(s, video=torch.zeros(40, H, W, 3, dtype=torch.uint8)) for s in samples])     # rgb frames: refused
    stager = D.ClipStager(len(samples), F.CLIP, H, W, F.CROP, channels=2)
    stager.submit(samples)
    clips, ssl = stager.collect(want_ssl=True)
    torch.cuda.synchronize()
    assert tuple(clips.shape) == tuple(ssl.shape) == (len(samples), 3, F.CLIP, F.CROP, F.CROP)
    assert is_zero_plane(clips) and is_zero_plane(ssl)
    for k in range(len(samples)):
        for got, key in ((clips, "clip"), (ssl, "ssl_clip")):
            g = got[k].cpu().numpy()
            assert np.array_equal(g[:2], fx[f"{key}_{k}"]), (k, key)
            assert (g[2] == 0).all() and not np.signbit(g[2]).any()
    assert int(fx["decision_0"][5]) < F.CLIP and (clips[0, :2, int(fx["decision_0"][5]):] == -1.0).all()      # the short window's padding


# ----------------------------------------------------------------------------- 3. Conv3d_1a: zero-plane path vs the generic chain
def _last_conv_kernel():
    from opental_amd import _lib as L
    return L.lib().otal_conv_last_kernel().decode()


@pytest.fixture(scope="module")
def flow_clip():
    """One flagged zero-plane batch (1,3,256,96,96) from uint8 flow frames, and the same clip as two planes."""
    from opental_amd.common.input_pipeline import prepare_clips
    g = torch.Generator().manual_seed(11)
    video = torch.randint(0, 256, (256, 96, 96, 2), generator=g, dtype=torch.uint8)
    clips, _ = prepare_clips([video], [0], 256, 96, decisions=[(0, 0, False)])
    return clips, clips[:, :2].contiguous()


@pytest.mark.parametrize("prec", [0, 1])
def test_conv3d_1a_on_a_zero_plane_batch_equals_the_two_channel_convolution(flow_clip, prec):
    """Forward output and weight gradient of the first layer at its own geometry (b = 1): the zero-plane path against the
    generic chain on the 2-plane clip (unchanged code, the yardstick).  Both round the same operands the same way and
    accumulate in fp32, so they differ by summation order only.
    fp32 (prec 0): the project's parity bar, 1e-4 of the tensor's largest magnitude, for both tensors.
    bf16 operands (prec 1): the forward keeps that bar (identical bf16 operands, fp32 accumulation over at most 1029 terms);
    the weight gradient takes the bound tests/test_bf16_layer_pin_gpu.py applies to an isolated layer's weight gradient.
    The Conv3d_1a kernels exist for bf16 operands only (csrc/conv_select.h: conv1a_direct_eligible / conv1a_wgrad_eligible need
    the precision bit), so the kernel names are asserted in that mode: the zero-plane path runs "conv1a" / "conv1a_wgrad",
    the 2-plane clip neither -- and in fp32 mode neither path does."""
    from test_bf16_layer_pin_gpu import BOUNDS, _cmp
    from opental_amd.common import ops
    from opental_amd.common.i3d_backbone import InceptionI3d
    from opental_amd.thumos14.BDNet import BDNet
    zero_plane, two_plane = flow_clip
    torch.manual_seed(4)
    model = InceptionI3d(final_endpoint='Conv3d_1a_7x7', in_channels=2)
    model.build()
    model.apply(BDNet.weight_init)
    model = model.cuda().eval()
    for p in model.parameters():
        p.requires_grad_(False)
    w = model.Conv3d_1a_7x7.conv3d.weight.requires_grad_(True)
    assert tuple(w.shape) == (64, 2, 7, 7, 7)
    dy = torch.randn(1, 64, 128, 48, 48, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    old = ops.CONV_PRECISION
    ops.CONV_PRECISION = prec
    res = []
    try:
        with torch.autograd.set_multithreading_enabled(False):      # the backward's launches on this thread: its last kernel is readable
            for x in (zero_plane, two_plane):
                w.grad = None
                y = model.extract_features(x, endpoints=('Conv3d_1a_7x7',))['Conv3d_1a_7x7']
                k_fwd = _last_conv_kernel()
                y.backward(dy)
                k_wgrad = _last_conv_kernel()
                torch.cuda.synchronize()
                res.append((y.detach(), w.grad.detach().clone(), k_fwd, k_wgrad))
    finally:
        ops.CONV_PRECISION = old
    (y3, g3, f3, b3), (y2, g2, f2, b2) = res
    print(f"prec {prec}: zero-plane kernels ({f3}, {b3}), 2-plane kernels ({f2}, {b2})")
    if prec:
        assert (f3, b3) == ("conv1a", "conv1a_wgrad"), (f3, b3)
    else:
        assert "conv1a" not in f3 and "conv1a" not in b3, (f3, b3)
    assert f2 and b2 and "conv1a" not in f2 and "conv1a" not in b2, (f2, b2)
    assert tuple(g3.shape) == tuple(g2.shape) == (64, 2, 7, 7, 7) and g3.is_contiguous()
    assert y3.dtype == y2.dtype == torch.float32 and y3.shape == y2.shape == dy.shape
    rel = lambda a, b: float((a - b).abs().max()) / float(b.abs().max())
    ey, eg = rel(y3, y2), rel(g3, g2)
    print(f"prec {prec}: forward max error / max magnitude {ey:.3e}, weight gradient {eg:.3e}; "
          f"weight gradient (norm error, cosine, rms error) {_cmp(g3, g2)}")
    assert ey < 1e-4, ey
    if prec:
        ne, cs, rms = _cmp(g3, g2)
        bn, bc, br = BOUNDS[("alone", "dw")]
        assert ne < bn and cs > bc and rms < br, ((ne, cs, rms), (bn, bc, br))
    else:
        assert eg < 1e-4, eg


# ----------------------------------------------------------------------------- 4. the trainer at b = 1
def _flow_trainer(dev, seed, lr=1e-4):
    import bench
    from opental_amd.thumos14.BDNet import BDNet
    from opental_amd.thumos14.multisegment_loss import MultiSegmentLoss
    from opental_amd.thumos14.train import DetectorTrainer
    torch.manual_seed(seed)
    net = BDNet(in_channels=2, training=False, use_edl=True)
    net.backbone._model.apply(BDNet.weight_init)
    net = net.to(dev).train()
    crit = MultiSegmentLoss(15, 0.5, 1.0, cls_loss_type='edl', edl_config=bench.EDL, os_head=True, act_config=bench.ACT).to(dev)
    crit.cls_loss.epoch = 12
    return DetectorTrainer(net, crit, bench.W, lr=lr, weight_decay=1e-3)


@pytest.mark.parametrize("prec", [0, 1])
def test_flow_trainer_arena_gradients_equal_plain_autograd(flow_clip, prec):
    """tests/test_train_gpu.py's test of the same name on BDNet(in_channels=2) fed a zero-plane batch: Conv3d_1a's gradient
    comes back from the backbone as a tensor (the extended weight is no arena parameter), loses its zero slice in
    ExtendWeightFunction.backward and must land in the (64,2,7,7,7) slot of the NaN-poisoned arena."""
    import bench
    from opental_amd.common import ops
    dev = torch.device("cuda", 0)
    clips = flow_clip[0]
    old = ops.CONV_PRECISION
    ops.CONV_PRECISION = prec
    try:
        tr = _flow_trainer(dev, seed=9)
        _, targets, scores = bench.synth_batch(1, 1000, dev)
        a = tr.arena
        w1a = tr.net.backbone._model.Conv3d_1a_7x7.conv3d.weight
        assert tuple(w1a.shape) == (64, 2, 7, 7, 7) and any(p is w1a for p in a.params)
        ibm = tr.criterion.cls_loss.weight_accum
        ibm0 = ibm.detach().clone()
        for _ in range(2):
            ibm.copy_(ibm0)
            a.grad.fill_(float("nan"))
            ops.activate_prologues(tr._prologues)
            try:
                cost, _ = tr.compute_cost(clips, targets, scores)
                tr.begin_backward()
                cost.backward()
                tr.end_backward()
            finally:
                ops.STEP.reset()
            got = a.grad.detach().clone()
        assert bool(torch.isfinite(got).all()), int((~torch.isfinite(got)).sum())
        assert tuple(w1a.grad.shape) == (64, 2, 7, 7, 7)
        for p in a.params:
            p.grad = None
        ibm.copy_(ibm0)
        cost2, _ = tr.compute_cost(clips, targets, scores)
        cost2.backward()
        worst = 0.0
        for p, off in zip(a.params, a.offsets):
            want = p.grad.reshape(-1)
            have = got[off:off + p.numel()]
            scale = float(want.abs().max()) + 1e-12
            worst = max(worst, float((have - want).abs().max()) / scale)
        assert float(w1a.grad.abs().max()) > 0
        assert worst < 1e-5, worst
    finally:
        ops.CONV_PRECISION = old


def test_flow_lane_graph_steps_equal_eager_steps(flow_clip):
    """The drivers' launch mode on the flow network: `launch = 'lanes'` runs the first plain step eagerly, captures the second
    and replays from then on.  Parameters and both Adam moments after one eager + three replayed steps are bit-identical to
    four eager steps; replayed_steps is asserted, so a silent fall-back to eager launches fails the test."""
    import bench
    from opental_amd.common import ops
    dev = torch.device("cuda", 0)
    clips = flow_clip[0]
    old = ops.CONV_PRECISION
    ops.CONV_PRECISION = 1
    try:
        rec = bench.synth_label_ring(1, 1000, dev, n=1)[0]

        def run(launch):
            tr = _flow_trainer(dev, seed=5)
            tr.launch = launch
            costs = [float(tr.step(clips, rec.targets, rec.scores)[0]) for _ in range(4)]
            torch.cuda.synchronize()
            assert tr.step_count == 4
            return tr, costs
        te, ce = run('eager')
        assert te.replayed_steps == 0
        tl, cl = run('lanes')
        assert tl.replayed_steps == 3 and tl.launch == 'lanes' and tl._graph[0] == "lanes"
        for name in ("flat", "m", "v"):
            a, b = getattr(te.arena, name), getattr(tl.arena, name)
            assert torch.equal(a, b), (name, float((a - b).abs().max()))
        assert ce == cl, (ce, cl)
        # a replay runs no forward check of its own: rgb frames into the captured flow step are refused all the same
        with pytest.raises(RuntimeError, match="other kind"):
            tl.step(clips.clone(), rec.targets, rec.scores)
    finally:
        ops.CONV_PRECISION = old


# ----------------------------------------------------------------------------- 5. checkpoint round trip into the test drivers
def test_flow_checkpoint_loads_into_the_test_drivers_and_runs_two_stream_detection(flow_clip, tmp_path):
    import bench
    from opental_amd.common import ops
    from opental_amd.common.driver import load_net
    from opental_amd.thumos14 import test as T
    from opental_amd.thumos14.BDNet import BDNet
    dev = torch.device("cuda", 0)
    old = ops.CONV_PRECISION
    ops.CONV_PRECISION = 1
    try:
        tr = _flow_trainer(dev, seed=3)
        _, targets, scores = bench.synth_batch(1, 1000, dev)
        tr.step(flow_clip[0], targets, scores)
        model_file, _ = tr.save_model(1, str(tmp_path / "ckpt"), str(tmp_path / "ckpt" / "training"))
        sd = torch.load(model_file, map_location="cpu")
        want = BDNet(in_channels=2, training=False, use_edl=True).state_dict()
        assert list(sd.keys()) == list(want.keys())
        assert all(tuple(sd[k].shape) == tuple(want[k].shape) for k in want)
        assert tuple(sd['backbone._model.Conv3d_1a_7x7.conv3d.weight'].shape) == (64, 2, 7, 7, 7)
        flow_net = load_net(BDNet, dev, False, model_file, in_channels=2, use_edl=True)
        assert torch.equal(flow_net.backbone._model.Conv3d_1a_7x7.conv3d.weight.cpu(),
                           sd['backbone._model.Conv3d_1a_7x7.conv3d.weight'])
        torch.manual_seed(8)
        rgb_net = BDNet(in_channels=3, training=False, use_edl=True)
        rgb_net.backbone._model.apply(BDNet.weight_init)
        rgb_net = rgb_net.to(dev).eval()
        g = torch.Generator(device="cuda").manual_seed(1)
        rgb = [torch.randint(0, 256, (3, 300, 96, 96), device="cuda", generator=g, dtype=torch.uint8)]
        flow = [torch.randint(0, 256, (2, 300, 96, 96), device="cuda", generator=g, dtype=torch.uint8)]
        rows, counts, _, dec = T.detect_batch(rgb_net, rgb, 10.0, flow_net=flow_net, flow_videos=flow)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(dec['score']).all()) and bool(torch.isfinite(dec['seg']).all())
        for r in (rows if isinstance(rows, (list, tuple)) else [rows]):
            assert bool(torch.isfinite(torch.as_tensor(r).float()).all())
    finally:
        ops.CONV_PRECISION = old


# ----------------------------------------------------------------------------- 6. the training driver on flow frames
def test_flow_train_driver_trains_resumes_and_refuses_rgb_frames(tmp_path):
    """python -m opental_amd.thumos14.train on a yaml with `model.in_channels: 2` and uint8 (T,H,W,2) frames: two epochs in one
    go equal one epoch plus a run resumed from its checkpoint, bit for bit (plain and ssl steps as the sampler draws them); the
    checkpoint holds the (64,2,7,7,7) first-layer weight; the same yaml pointed at rgb frames is refused before any step."""
    import sys
    import yaml
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    from make_synthetic_thumos import make
    from opental_amd.common import ops
    from opental_amd.thumos14 import train as R
    rgb_yaml = make(str(tmp_path / "data"), videos=2, frames=400, size=100)
    flow_dir = tmp_path / "data" / "train_flow_npy"
    flow_dir.mkdir()
    for fn in os.listdir(tmp_path / "data" / "train_npy"):
        np.save(flow_dir / fn, np.ascontiguousarray(np.load(tmp_path / "data" / "train_npy" / fn)[..., :2]))
    cfg = yaml.safe_load(open(rgb_yaml))
    cfg["model"]["in_channels"] = 2
    mixed_yaml = str(tmp_path / "data" / "flow_model_rgb_frames.yaml")
    yaml.dump(cfg, open(mixed_yaml, "w"))
    cfg["dataset"]["training"]["video_data_path"] = str(flow_dir)
    flow_yaml = str(tmp_path / "data" / "flow.yaml")
    yaml.dump(cfg, open(flow_yaml, "w"))
    flags = ['--open_set', '--split', '0', '--lw', '1', '--cw', '10', '--piou', '0.5', '--ssl', '0.001', '--batch_size', '2',
             '--random_init', '--save_after', '0', '--max_steps', '2']
    old = ops.CONV_PRECISION
    try:
        tr_a, hist_a = R.main([flow_yaml] + flags + ['--max_epoch', '2', '--checkpoint_path', str(tmp_path / "run_a")])
        assert len(hist_a) == 2 and all(np.isfinite(h).all() for h in hist_a) and tr_a.step_count == 4
        sd = torch.load(tmp_path / "run_a" / "checkpoint-2.ckpt", map_location="cpu")
        assert tuple(sd['backbone._model.Conv3d_1a_7x7.conv3d.weight'].shape) == (64, 2, 7, 7, 7)
        R.main([flow_yaml] + flags + ['--max_epoch', '1', '--checkpoint_path', str(tmp_path / "run_b")])
        tr_b, hist_b = R.main([flow_yaml] + flags + ['--max_epoch', '2', '--resume', '1', '--checkpoint_path', str(tmp_path / "run_b")])
        assert len(hist_b) == 1 and tr_b.step_count == 4
        assert torch.equal(tr_a.arena.flat, tr_b.arena.flat) and hist_b[0] == hist_a[1]
        with pytest.raises(SystemExit, match="in_channels"):
            R.main([mixed_yaml] + flags + ['--max_epoch', '1', '--checkpoint_path', str(tmp_path / "run_c")])
    finally:
        ops.CONV_PRECISION = old
