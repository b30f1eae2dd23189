"""GPU: otal_decode_clips_2s -- the decode launch of a two-stream run, which reads the rgb and the flow network's raw maps and
averages them in registers -- against the route it replaces: fuse_outputs (torch's (rgb + flow) / 2.0 per map) followed by
otal_decode_clips_ev, with rpl_logits' negation for the GCPL decode.

The contract is bitwise: seg, score, actn and flag are torch.equal, and unct is
((unct_rgb + unct_flow) / 2 + (prop_unct_rgb + prop_unct_flow) / 2) / 2 as torch computes it when the four uncertainty maps
are given, otal_decode_clips_ev's own unct on the fused maps when they are not.  All inputs are normal finite floats.

Mixed flags: every case is run at three thresholds -- 0.01, and half of and the whole median of the reference's scores (taken
from otal_decode_clips_ev on the fused maps, not from the entry under test) -- and for at least one of them
0 < flag.sum() < flag.numel() must hold.  A case with ONE flag (one clip, one anchor, one class) cannot mix within a launch:
there the flag must be set at one threshold and clear at another."""
import pytest
import torch

pytestmark = pytest.mark.gpu
E_NULL, E_SHAPE, E_UNSUPPORTED = -1, -2, -7
MAPS = ("loc", "prop_loc", "conf", "prop_conf", "center")
CLIP = 256.0

# (name, os_head, score_fn, first_class, evidence, conf_sign, K)
HEADS = [(f"opental-{ev}-K{K}", True, 0, 0, e, 1, K) for K in (1, 15) for e, ev in enumerate(("exp", "relu", "softplus"))] + \
        [(f"edl-{ev}-C{C}", False, 0, 1, e, 1, C) for C in (2, 21) for e, ev in enumerate(("exp", "relu", "softplus"))] + \
        [(f"softmax-C{C}", False, 1, 1, 0, 1, C) for C in (2, 21)] + \
        [(f"gcpl-C{C}", False, 1, 1, 0, -1, C) for C in (2, 21)]


def _lib():
    from opental_amd import _lib as L
    return L


def _network(g, n, A, K, os_head, sure):
    """One network's raw maps.  loc has both signs and a spread wider than the clip, so both clamps of decode_segment fire;
    the actionness logits have both signs (`sure`: positive, for the cases of one anchor in one clip)."""
    dev = "cuda"
    r = lambda *s: torch.randn(*s, device=dev, generator=g)
    out = dict(loc=r(n, A, 2) * 150.0, prop_loc=r(n, A, 2), conf=r(n, A, K) * 2.0, prop_conf=r(n, A, K) * 2.0, center=r(n, A, 1))
    if os_head:
        # every other anchor has actionness logits > 0 in both networks, the ones between < 0: flags of both kinds
        sign = 1.0 if sure else 1.0 - 2.0 * (torch.arange(n * A, device=dev) % 2).view(n, A, 1)
        out.update(act=(r(n, A, 1).abs() + 0.1) * sign, prop_act=(r(n, A, 1).abs() + 0.1) * sign)
    out.update(unct=torch.rand(n, A, device=dev, generator=g) * 0.9 + 0.05,
               prop_unct=torch.rand(n, A, device=dev, generator=g) * 0.9 + 0.05)
    return out


def _pair(seed, n, A, K, os_head):
    g = torch.Generator(device="cuda").manual_seed(seed)
    sure = n * A == 1
    rgb, flow = _network(g, n, A, K, os_head, sure), _network(g, n, A, K, os_head, sure)
    priors = ((torch.arange(A, device="cuda", dtype=torch.float32) + 0.5) / A).view(A, 1)
    offsets = torch.tensor([0.0, 128.0, 517.0][:n], device="cuda")
    fps = torch.tensor([10.0, 7.5, 30.0][:n], device="cuda")
    for d in (rgb, flow):
        d["priors"] = priors
        assert all(bool(torch.isfinite(v).all()) and bool((v.abs() >= 2.0 ** -126).all()) for v in d.values())
    return rgb, flow, offsets, fps


class Outputs(object):
    """The five outputs, pre-filled with a sentinel."""

    def __init__(self, n, A, KO, sentinel=None):
        new = torch.empty if sentinel is None else lambda *s, **k: torch.full(s[0], sentinel, **k)
        self.seg = new((n, A, 2), device="cuda")
        self.score = new((n, KO, A), device="cuda")
        self.unct = new((n, A), device="cuda")
        self.actn = new((n, A), device="cuda")
        self.flag = new((n, KO, A), device="cuda", dtype=torch.uint8)
        self.sentinel = sentinel

    def ptrs(self):
        p = _lib().ptr
        return p(self.seg), p(self.score), p(self.unct), p(self.actn), p(self.flag)

    def intact(self):
        torch.cuda.synchronize()
        return all(bool((t == self.sentinel).all()) for t in (self.seg, self.score, self.unct, self.actn, self.flag))


def _shape(maps):
    n, A, _ = maps["loc"].shape
    return n, A, maps["conf"].shape[-1]


def run_ev(maps, offsets, fps, thresh, score_fn, first, evidence, out=None):
    """otal_decode_clips_ev on one network's (or the fused) maps."""
    L = _lib()
    n, A, K = _shape(maps)
    out = out or Outputs(n, A, K - first)
    p = lambda k: L.ptr(maps[k]) if maps.get(k) is not None else None
    assert all(maps[k].is_contiguous() for k in MAPS)
    rc = L.lib().otal_decode_clips_ev(p("loc"), p("prop_loc"), L.ptr(maps["priors"]), p("conf"), p("prop_conf"), p("center"),
                                      p("act"), p("prop_act"), L.ptr(offsets), L.ptr(fps), *out.ptrs(), n, A, K, CLIP, thresh,
                                      score_fn, first, evidence, L.stream())
    return rc, out


def run_2s(rgb, flow, offsets, fps, thresh, score_fn, first, evidence, sign, with_unct=True, out=None, override=None):
    """otal_decode_clips_2s.  override: {argument name: value} (None for a null pointer), e.g. dict(flow_conf=None, K=0)."""
    L = _lib()
    override = override or {}
    n, A, K = _shape(rgb)
    out = out or Outputs(n, A, max(K - first, 1))
    args = {}
    for prefix, d in (("", rgb), ("flow_", flow)):
        for k in MAPS + ("act", "prop_act"):
            args[prefix + k] = L.ptr(d[k]) if d.get(k) is not None else None
    for name, d, k in (("unct_in", rgb, "unct"), ("prop_unct_in", rgb, "prop_unct"), ("flow_unct_in", flow, "unct"),
                       ("flow_prop_unct_in", flow, "prop_unct")):
        args[name] = L.ptr(d[k]) if with_unct else None
    args.update(nclips=n, A=A, K=K, score_fn=score_fn, first_class=first, evidence=evidence, conf_sign=sign)
    assert set(override) <= set(args), override
    args.update(override)
    a = args
    rc = L.lib().otal_decode_clips_2s(
        a["loc"], a["prop_loc"], a["conf"], a["prop_conf"], a["center"], a["act"], a["prop_act"], a["flow_loc"],
        a["flow_prop_loc"], a["flow_conf"], a["flow_prop_conf"], a["flow_center"], a["flow_act"], a["flow_prop_act"],
        a["unct_in"], a["prop_unct_in"], a["flow_unct_in"], a["flow_prop_unct_in"], L.ptr(rgb["priors"]), L.ptr(offsets),
        L.ptr(fps), *out.ptrs(), a["nclips"], a["A"], a["K"], CLIP, thresh, a["score_fn"], a["first_class"], a["evidence"],
        a["conf_sign"], L.stream())
    return rc, out


def _fused(rgb, flow, sign):
    from opental_amd.common.detect import fuse_outputs, rpl_logits
    return rpl_logits(fuse_outputs(rgb, flow), sign == -1)


def _own_unct(rgb, flow):
    return ((rgb["unct"] + flow["unct"]) / 2.0 + (rgb["prop_unct"] + flow["prop_unct"]) / 2.0) / 2.0


@pytest.mark.parametrize("A", [1, 126, 130])
@pytest.mark.parametrize("head", HEADS, ids=[h[0] for h in HEADS])
def test_bitwise_equal_to_decoding_the_fused_maps(head, A):
    name, os_head, score_fn, first, evidence, sign, K = head
    for n in (1, 3):
        rgb, flow, offsets, fps = _pair(1000 * A + 10 * K + n, n, A, K, os_head)
        fused = _fused(rgb, flow, sign)
        rc, probe = run_ev(fused, offsets, fps, 0.01, score_fn, first, evidence)
        assert rc == 0
        median = float(probe.score.median())
        assert 0.0 < median < 1.0
        flags, clamps = [], torch.zeros(2, dtype=torch.bool)
        for thresh in (0.01, 0.5 * median, median):
            rc, want = run_ev(fused, offsets, fps, thresh, score_fn, first, evidence)
            assert rc == 0
            for with_unct in ((True, False) if score_fn == 0 else (False,)):
                rc, got = run_2s(rgb, flow, offsets, fps, thresh, score_fn, first, evidence, sign, with_unct)
                assert rc == 0, (name, n, thresh, with_unct)
                assert torch.equal(got.seg, want.seg), (name, n, thresh)
                assert torch.equal(got.score, want.score), (name, n, thresh)
                assert torch.equal(got.flag, want.flag), (name, n, thresh)
                if os_head:
                    assert torch.equal(got.actn, want.actn), (name, n, thresh)
                assert torch.equal(got.unct, _own_unct(rgb, flow) if with_unct else want.unct), (name, n, thresh, with_unct)
            flags.append(want.flag)
            start = want.seg * fps.view(n, 1, 1) - offsets.view(n, 1, 1)          # frames inside the clip, up to rounding
            clamps |= torch.stack([(start.abs() < 1e-2).any(), ((start - CLIP).abs() < 1e-2).any()]).cpu()
        if flags[0].numel() > 1:
            assert any(0 < int(f.sum()) < f.numel() for f in flags), (name, n, [int(f.sum()) for f in flags])
        else:
            assert {int(f.sum()) for f in flags} == {0, 1}, (name, n)
        if n * A >= 126:
            assert bool(clamps.all()), (name, n)             # both clamps of decode_segment fired


def test_unct_is_zero_under_softmax_without_the_maps_and_the_average_with_them():
    rgb, flow, offsets, fps = _pair(5, 3, 130, 21, False)
    rc, got = run_2s(rgb, flow, offsets, fps, 0.01, 1, 1, 0, 1, with_unct=False, out=Outputs(3, 130, 20, 7.0))
    assert rc == 0 and bool((got.unct == 0).all())
    rc, got = run_2s(rgb, flow, offsets, fps, 0.01, 1, 1, 0, 1, with_unct=True)
    assert rc == 0 and torch.equal(got.unct, _own_unct(rgb, flow))


@pytest.mark.parametrize("head", [HEADS[3], HEADS[5], HEADS[10], HEADS[13]], ids=lambda h: h[0])
def test_the_same_tensors_for_both_streams_decode_as_one_network(head):
    """(x + x) / 2 == x exactly: the two-stream launch on (x, x) is otal_decode_clips_ev on x.  No fuse_outputs here."""
    name, os_head, score_fn, first, evidence, sign, K = head
    rgb, _, offsets, fps = _pair(77, 3, 130, K, os_head)
    rc, want = run_ev(rgb, offsets, fps, 0.05, score_fn, first, evidence)
    rc2, got = run_2s(rgb, dict(rgb), offsets, fps, 0.05, score_fn, first, evidence, 1, with_unct=False)
    assert rc == 0 and rc2 == 0
    for k in ("seg", "score", "unct", "actn", "flag") if os_head else ("seg", "score", "unct", "flag"):
        assert torch.equal(getattr(got, k), getattr(want, k)), (name, k)
    assert 0 < int(want.flag.sum()) < want.flag.numel()


def test_decision_edges_of_the_fused_actionness():
    """Anchors whose flow actionness logits are the negated rgb ones: the fused logits are exactly 0, the actionness exactly
    0.5, and `actionness > 0.5` is strict -- never flagged, whatever the score.  The neighbour with fused logits +2^-20 has
    sigmoid(2^-20) > 0.5 in fp32 and is flagged once its score passes."""
    n, A, K = 1, 8, 15
    rgb, flow, offsets, fps = _pair(3, n, A, K, True)
    for k in ("act", "prop_act"):
        flow[k][0, :4] = -rgb[k][0, :4]
        rgb[k][0, 4] = 1.0
        flow[k][0, 4] = -1.0 + 2.0 ** -19            # 1 + (-1 + 2^-19) = 2^-19 exactly; halved: 2^-20
        assert float((rgb[k][0, 4] + flow[k][0, 4]) / 2.0) == 2.0 ** -20
    rc, got = run_2s(rgb, flow, offsets, fps, -1.0, 0, 0, 0, 1)                    # every score passes -1
    assert rc == 0
    assert bool((got.actn[0, :4] == 0.5).all()) and int(got.flag[0, :, :4].sum()) == 0
    assert float(got.actn[0, 4]) > 0.5 and int(got.flag[0, :, 4].sum()) == K
    assert bool((got.score[0, :, :5] > 0).all())
    rc, got = run_2s(rgb, flow, offsets, fps, 2.0, 0, 0, 0, 1)                     # no score passes 2
    assert rc == 0 and int(got.flag.sum()) == 0
    rc, want = run_ev(_fused(rgb, flow, 1), offsets, fps, -1.0, 0, 0, 0)
    rc, got = run_2s(rgb, flow, offsets, fps, -1.0, 0, 0, 0, 1)
    assert torch.equal(got.flag, want.flag) and torch.equal(got.actn, want.actn)


def test_refused_calls_return_their_code_and_write_nothing():
    n, A, K = 3, 130, 15
    rgb, flow, offsets, fps = _pair(9, n, A, K, True)
    refusals = [(dict(flow_conf=None), E_NULL),                                     # a null flow map
                (dict(flow_loc=None), E_NULL),
                (dict(flow_act=None, flow_prop_act=None), E_NULL),                  # act given for one stream only
                (dict(act=None, prop_act=None), E_NULL),
                (dict(flow_prop_unct_in=None), E_NULL),                             # three of the four uncertainty maps
                (dict(unct_in=None), E_NULL),
                (dict(evidence=3), E_UNSUPPORTED),
                (dict(score_fn=2), E_UNSUPPORTED),
                (dict(conf_sign=0), E_UNSUPPORTED),
                (dict(conf_sign=2), E_UNSUPPORTED),
                (dict(K=0), E_SHAPE),                                               # K < 1
                (dict(K=1, first_class=1), E_SHAPE),                                # no class left
                (dict(nclips=0), E_SHAPE)]
    for override, code in refusals:
        out = Outputs(n, A, K, sentinel=7.0)
        rc, _ = run_2s(rgb, flow, offsets, fps, 0.01, 0, 0, 0, 1, out=out, override=override)
        assert rc == code, (override, rc)
        assert out.intact(), override
    out = Outputs(n, A, K, sentinel=7.0)
    rc, _ = run_2s(rgb, flow, offsets, fps, 0.01, 0, 0, 0, 1, out=out)              # the same call, not refused, writes them all
    assert rc == 0
    torch.cuda.synchronize()
    assert not bool((out.seg == 7.0).any()) and not bool((out.score == 7.0).any()) and not bool((out.flag == 7).any())
    assert not bool((out.unct == 7.0).any()) and not bool((out.actn == 7.0).any())


def test_decode_clips_two_stream_returns_decode_clips_dict_and_refuses_what_it_must():
    from opental_amd.common import detect as D
    rgb, flow, offsets, fps = _pair(21, 3, 126, 15, True)
    got = D.decode_clips_two_stream(rgb, flow, offsets, fps, 256, 0.05)
    fused = D.fuse_outputs(rgb, flow)
    want = D.decode_clips(fused, offsets, fps, 256, 0.05)
    want["unct"] = ((fused["unct"] + fused["prop_unct"]) / 2.0).contiguous()
    assert sorted(got) == sorted(want)
    for k in want:
        assert torch.equal(got[k], want[k]), k
    no_act = lambda d: {k: v for k, v in d.items() if k not in ("act", "prop_act")}
    closed = no_act(rgb), no_act(flow)
    got = D.decode_clips_two_stream(*closed, offsets, fps, 256, 0.05, os_head=False, use_edl=False, use_gcpl=True)
    want = D.decode_clips(D.fuse_outputs(*closed), offsets, fps, 256, 0.05, os_head=False, use_edl=False, use_gcpl=True)
    assert got["unct"] is None and got["actn"] is None
    assert all(torch.equal(got[k], want[k]) for k in ("seg", "score", "flag"))
    with pytest.raises(NotImplementedError):
        D.decode_clips_two_stream(rgb, flow, offsets, fps, os_head=True, use_edl=False)
    with pytest.raises(NotImplementedError):
        D.decode_clips_two_stream(rgb, flow, offsets, fps, use_gcpl=True)
    with pytest.raises(NotImplementedError):
        D.decode_clips_two_stream(rgb, flow, offsets, fps, evidence="tanh")
    with pytest.raises(RuntimeError, match="conf"):
        narrow = dict(flow, conf=flow["conf"][:, :, :14], prop_conf=flow["prop_conf"][:, :, :14])
        D.decode_clips_two_stream(rgb, narrow, offsets, fps)
    with pytest.raises(RuntimeError, match="priors"):
        D.decode_clips_two_stream(rgb, dict(flow, priors=flow["priors"] + 0.25), offsets, fps)
    with pytest.raises(RuntimeError, match="device"):
        D.decode_clips_two_stream({k: v.cpu() for k, v in rgb.items()}, flow, offsets, fps)
    with pytest.raises(RuntimeError, match="unct"):
        D.decode_clips_two_stream(rgb, {k: v for k, v in flow.items() if k != "unct"}, offsets, fps)


def _two_networks():
    from opental_amd.thumos14.BDNet import BDNet
    torch.manual_seed(0)
    nets = []
    for cin in (3, 2):
        net = BDNet(in_channels=cin, training=False, use_edl=True)
        net.backbone._model.apply(BDNet.weight_init)
        nets.append(net.cuda().eval())
    g = torch.Generator(device="cuda").manual_seed(1)
    rgb = [torch.randint(0, 256, (3, 300, 96, 96), device="cuda", generator=g, dtype=torch.uint8)]
    flow = [torch.randint(0, 256, (2, 300, 96, 96), device="cuda", generator=g, dtype=torch.uint8)]
    return nets, rgb, flow


def test_detect_batch_routes_agree_and_the_default_one_never_fuses(monkeypatch):
    """Two small random BDNets (3 and 2 input channels), one 300-frame video each: detect_batch's default route (raw maps of
    both networks into one decode launch) against two_stream_decode=False (fuse_outputs per chunk, decode_clips, uncertainty
    substituted) -- rows, counts, index and every tensor of dec torch.equal; and with fuse_outputs failing the test, the
    default route still runs."""
    from opental_amd.common import detect as D, ops
    from opental_amd.thumos14 import test as T
    old = ops.CONV_PRECISION
    ops.CONV_PRECISION = 1
    try:
        nets, rgb, flow = _two_networks()
        old_route = T.detect_batch(nets[0], rgb, 10.0, flow_net=nets[1], flow_videos=flow, two_stream_decode=False)
        monkeypatch.setattr(D, "fuse_outputs", lambda *a, **k: pytest.fail("the default route must not call fuse_outputs"))
        new_route = T.detect_batch(nets[0], rgb, 10.0, flow_net=nets[1], flow_videos=flow)
        for a, b, what in zip(old_route[:3], new_route[:3], ("rows", "counts", "index")):
            assert torch.equal(a, b), what
        assert sorted(old_route[3]) == sorted(new_route[3])
        for k, v in old_route[3].items():
            assert v.shape == new_route[3][k].shape and torch.equal(v, new_route[3][k]), k
        assert int(new_route[1].sum()) > 0 and 0 < int(new_route[3]["flag"].sum()) < new_route[3]["flag"].numel()
    finally:
        ops.CONV_PRECISION = old
