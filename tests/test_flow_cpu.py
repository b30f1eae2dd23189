"""CPU: the optical-flow stream's training side, as far as it goes without a GPU -- the new C entry's declaration, export and
argument checks (otal_prepare_clips_ch, csrc/input.hip), the 2-channel host input path (load_video_data, THUMOS_Dataset.
decide against tests/golden/flow_dataset.npz, written by tools/pin_flow_dataset.py from the reference's own
THUMOS_Dataset.__getitem__), the zero-slice weight extension (common/i3d_backbone.ExtendWeightFunction) and the refusals: rgb
frames into a flow network, flow frames into an rgb network, ActivityNet flow training."""
import ctypes
import os
import random
import re

import numpy as np
import pytest
import torch

import flow_cases as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from opental_amd.csrc import build
    if not os.path.exists(build.LIB):
        build.build(verbose=False)
    from opental_amd._lib import declare
    return declare(ctypes.CDLL(build.LIB))


def test_header_declares_and_library_exports_prepare_clips_ch(lib):
    txt = open(os.path.join(REPO, "include", "opental_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"int\s+otal_prepare_clips_ch\s*\(([^)]*)\)", txt)
    assert m, "include/opental_hip.h does not declare otal_prepare_clips_ch"
    args = [a.strip() for a in m.group(1).split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ["frames", "params", "frame_map", "out", "out_ssl", "B", "C_src", "C_out",
                                                         "T", "Hs", "Ws", "Ho", "Wo", "stream"]
    assert hasattr(lib, "otal_prepare_clips_ch")
    assert hasattr(lib, "otal_prepare_clips") and hasattr(lib, "otal_prepare_clips_map")       # the two older entries stay


def test_prepare_clips_ch_argument_errors_do_not_launch(lib):
    one = ctypes.c_void_p(16)       # never dereferenced: argument checks come first
    f = ctypes.cast(one, ctypes.POINTER(ctypes.c_float))
    call = lib.otal_prepare_clips_ch
    shape = (1, 2, 3, 4, 8, 8, 4, 4)            # B, C_src, C_out, T, Hs, Ws, Ho, Wo
    assert call(None, one, one, f, f, *shape, None) == -1                   # frames
    assert call(one, None, one, f, f, *shape, None) == -1                   # params
    assert call(one, one, one, None, None, *shape, None) == -1              # both outputs
    assert call(one, one, None, f, f, *shape, None) == -1                   # out_ssl without a frame map
    assert call(one, one, None, None, f, *shape, None) == -1
    assert call(one, one, one, f, f, 1, 2, 3, 4, 8, 8, 9, 4, None) == -2    # Ho > Hs
    assert call(one, one, one, f, f, 1, 2, 3, 4, 8, 8, 4, 9, None) == -2    # Wo > Ws
    assert call(one, one, one, f, f, 0, 2, 3, 4, 8, 8, 4, 4, None) == -2
    for cs, co in ((1, 3), (4, 4), (3, 2), (2, 4)):
        assert call(one, one, one, f, f, 1, cs, co, 4, 8, 8, 4, 4, None) == -7, (cs, co)
    assert lib.otal_abi_version() == 26         # an additive entry


def test_load_video_data_takes_two_and_three_channels_only(tmp_path):
    from opental_amd.common import thumos_dataset as D
    rs = np.random.RandomState(0)

    def load(arr):
        d = tmp_path / f"v{arr.shape[-1]}_{arr.dtype}"
        d.mkdir()
        np.save(d / "vid.npy", arr)
        return D.load_video_data({"vid": {}}, str(d), pin=False)["vid"]
    flow = rs.randint(0, 256, (7, 5, 6, 2)).astype(np.uint8)
    got = load(flow)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (7, 5, 6, 2) and np.array_equal(got.numpy(), flow)
    assert tuple(load(rs.randint(0, 256, (7, 5, 6, 3)).astype(np.uint8)).shape) == (7, 5, 6, 3)
    for c in (1, 4):
        with pytest.raises(RuntimeError):
            load(rs.randint(0, 256, (7, 5, 6, c)).astype(np.uint8))
    with pytest.raises(RuntimeError):
        load(rs.rand(7, 5, 6, 2).astype(np.float32))


def _dataset(videos, infos, annos):
    from opental_amd.common import thumos_dataset as D
    data = {n: torch.from_numpy(v) for n, v in videos.items()}
    return D.THUMOS_Dataset(data, infos, annos, clip_length=F.CLIP, crop_size=F.CROP, stride=F.STRIDE)


def test_decide_draws_the_same_random_sequence_for_two_and_three_channels():
    frames = F.make_frames()
    infos, annos, flow_videos = F.dataset_tables(frames)
    rgb_videos = {n: np.concatenate([v, v[..., :1]], -1) for n, v in flow_videos.items()}      # equal frame size, 3 channels
    flow_ds, rgb_ds = _dataset(flow_videos, infos, annos), _dataset(rgb_videos, infos, annos)
    assert len(flow_ds) == len(rgb_ds) >= 3
    flips, flags = set(), set()
    for seed in range(6):
        for idx in range(len(flow_ds)):
            random.seed(seed)
            a = flow_ds.decide(idx)
            after_a = random.random()
            random.seed(seed)
            b = rgb_ds.decide(idx)
            assert random.random() == after_a                       # the same number of draws
            assert a['crop'] == b['crop'] and a['offset'] == b['offset'] and a['flag'] == b['flag']
            assert (a['frame_map'] is None) == (b['frame_map'] is None)
            assert a['frame_map'] is None or np.array_equal(a['frame_map'], b['frame_map'])
            for k in ('target', 'ssl_target', 'scores'):
                assert np.array_equal(a[k], b[k]), k
            assert a['video'].shape[3] == 2 and b['video'].shape[3] == 3
            flips.add(bool(a['crop'][2]))
            flags.add(bool(a['flag']))
    assert flips == {False, True} and flags == {False, True}        # both outcomes of both decisions were compared


def test_decisions_equal_the_reference_fixture(golden_dir):
    fx = np.load(os.path.join(golden_dir, "flow_dataset.npz"))
    assert np.array_equal(fx["frames"], F.make_frames())
    infos, annos, videos = F.dataset_tables(fx["frames"])
    ds = _dataset(videos, infos, annos)
    seen = []
    for k, (idx, seed) in enumerate(fx["picks"]):
        random.seed(int(seed))
        d = ds.decide(int(idx))
        i, j, flip, offset, flag, valid = (int(v) for v in fx[f"decision_{k}"])
        assert (d['crop'], d['offset'], bool(d['flag'])) == ((i, j, bool(flip)), offset, bool(flag))
        assert min(F.CLIP, d['video'].shape[0] - d['offset']) == valid
        fm = fx[f"map_{k}"]
        assert (d['frame_map'] is None) == (fm.size == 0) and (fm.size == 0 or np.array_equal(d['frame_map'], fm))
        assert np.array_equal(d['target'], fx[f"target_{k}"]) and np.array_equal(d['ssl_target'], fx[f"ssl_target_{k}"])
        assert fx[f"clip_{k}"].shape == fx[f"ssl_clip_{k}"].shape == (2, F.CLIP, F.CROP, F.CROP)
        seen.append((bool(flip), bool(flag), valid < F.CLIP))
    assert len(seen) == 4 and any(s[0] for s in seen) and any(s[1] for s in seen) and any(s[2] for s in seen)


def test_extended_weight_has_an_exactly_zero_third_slice_and_the_right_gradient():
    from opental_amd.common.i3d_backbone import ExtendWeightFunction
    g = torch.Generator().manual_seed(3)
    w = torch.randn(4, 2, 3, 3, 3, dtype=torch.float64, generator=g, requires_grad=True)
    buf = torch.zeros(4, 3, 3, 3, 3, dtype=torch.float64)
    out = ExtendWeightFunction.apply(w, buf)
    assert tuple(out.shape) == (4, 3, 3, 3, 3) and torch.equal(out[:, :2], w.detach())
    third = out[:, 2]
    assert bool((third == 0).all()) and not bool(torch.signbit(third).any())
    assert out.data_ptr() == buf.data_ptr() and buf.grad_fn is None and not buf.requires_grad      # the graph is not parked on the buffer
    up = torch.randn(4, 3, 3, 3, 3, dtype=torch.float64, generator=g)
    (gw,) = torch.autograd.grad(out, w, up)
    assert tuple(gw.shape) == (4, 2, 3, 3, 3) and gw.is_contiguous() and torch.equal(gw, up[:, :2])
    assert torch.autograd.gradcheck(lambda t: ExtendWeightFunction.apply(t, buf), (w,))
    assert bool((buf[:, 2] == 0).all())
    with pytest.raises(RuntimeError):
        ExtendWeightFunction.apply(torch.randn(4, 3, 3, 3, 3, dtype=torch.float64), buf)


def _stem(in_channels):
    from opental_amd.common.i3d_backbone import InceptionI3d
    m = InceptionI3d(final_endpoint='Conv3d_1a_7x7', in_channels=in_channels)
    m.build()
    return m.eval().requires_grad_(False)


def test_rgb_frames_into_a_flow_network_and_flow_frames_into_an_rgb_network_raise():
    from opental_amd.common.input_pipeline import mark_zero_plane
    flow_net, rgb_net = _stem(2), _stem(3)
    rgb_clip, flow_clip = torch.zeros(1, 3, 8, 16, 16), torch.zeros(1, 2, 8, 16, 16)
    with pytest.raises(RuntimeError, match="not flagged as a zero-plane"):
        flow_net.extract_features(rgb_clip, endpoints=('Conv3d_1a_7x7',))
    with pytest.raises(RuntimeError, match="2 planes"):
        rgb_net.extract_features(flow_clip, endpoints=('Conv3d_1a_7x7',))
    with pytest.raises(RuntimeError, match="zero-plane optical-flow batch"):
        rgb_net.extract_features(mark_zero_plane(torch.zeros(1, 3, 8, 16, 16)), endpoints=('Conv3d_1a_7x7',))
    with pytest.raises(RuntimeError, match="4 planes"):
        flow_net.extract_features(torch.zeros(1, 4, 8, 16, 16), endpoints=('Conv3d_1a_7x7',))


def test_trainer_input_clones_keep_the_zero_plane_flag():
    from opental_amd.common.input_pipeline import is_zero_plane, mark_zero_plane
    from opental_amd.thumos14.train import _clone_inputs
    scores = torch.zeros(1, 2, 8)
    c, _, _ = _clone_inputs(mark_zero_plane(torch.zeros(1, 3, 8, 4, 4)), None, scores)
    assert is_zero_plane(c)
    c, _, _ = _clone_inputs(torch.zeros(1, 3, 8, 4, 4), None, scores)
    assert not is_zero_plane(c)


def test_flow_config_differs_from_the_rgb_config_where_it_should():
    import yaml
    rgb = yaml.safe_load(open(os.path.join(REPO, "configs", "thumos14_opental_final.yaml")))
    flow = yaml.safe_load(open(os.path.join(REPO, "configs", "thumos14_opental_flow.yaml")))

    def leaves(d, pre=()):
        for k, v in d.items():
            if isinstance(v, dict) and pre + (k,) != ('training', 'edl_config') and pre + (k,) != ('training', 'act_config'):
                yield from leaves(v, pre + (k,))
            else:
                yield pre + (k,), v
    a, b = dict(leaves(rgb)), dict(leaves(flow))
    assert a.keys() == b.keys()
    assert {k for k in a if a[k] != b[k]} == {
        ('model', 'in_channels'), ('model', 'backbone_model'), ('dataset', 'training', 'video_data_path'),
        ('dataset', 'testing', 'video_data_path'), ('training', 'checkpoint_path'), ('testing', 'checkpoint_path'),
        ('testing', 'output_path')}
    assert flow['model']['in_channels'] == 2 and flow['model']['backbone_model'].endswith('flow_imagenet.pt')
    assert 'validation_flow_npy' in flow['dataset']['training']['video_data_path']
    assert 'test_flow_npy' in flow['dataset']['testing']['video_data_path']
    assert 'thumos14_flow' in flow['training']['checkpoint_path'] and 'thumos14_flow' in flow['testing']['checkpoint_path']


def test_driver_refuses_frames_of_the_other_stream():
    from opental_amd.thumos14.train import check_stream_channels
    assert check_stream_channels({'model': {'in_channels': 2}}, torch.zeros(4, 5, 6, 2, dtype=torch.uint8)) == 2
    assert check_stream_channels({'model': {'in_channels': 3}}, torch.zeros(4, 5, 6, 3, dtype=torch.uint8)) == 3
    with pytest.raises(SystemExit):
        check_stream_channels({'model': {'in_channels': 2}}, torch.zeros(4, 5, 6, 3, dtype=torch.uint8))
    with pytest.raises(SystemExit):
        check_stream_channels({'model': {'in_channels': 3}}, torch.zeros(4, 5, 6, 2, dtype=torch.uint8))


def test_anet_training_refuses_a_two_channel_model():
    from opental_amd.anet.train import build_training
    from opental_amd.common import config as C
    cfg = C.get_config([os.path.join(REPO, "configs", "anet_opental.yaml"), "--open_set", "--split", "0",
                        "--lw", "1", "--cw", "1", "--piou", "0.6", "--ssl", "0.1"])
    cfg['model']['in_channels'] = 2
    with pytest.raises(RuntimeError, match="in_channels"):
        build_training(cfg, torch.device("cpu"), random_init=True)
