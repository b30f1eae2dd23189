"""CPU: the closed-set Softmax and EDL baselines (os_head false) against tests/golden/closed_set.npz, written from the
reference by tools/pin_closed_set.py -- MultiSegmentLoss terms and gradients, the result rows of get_video_detections,
and the argument checks of the new C entry points (no launch)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import arch

C = 16
EDL_CFG = dict(evidence='exp', loss_type='log', soft_label=0, with_focal=False, alpha=0.25, gamma=2)


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "closed_set.npz"))


def head_outputs(B=2, seed=31):
    """The synthetic head outputs of tools/pin_closed_set.py (same seed, same draws)."""
    rs = np.random.RandomState(seed)
    K = sum(arch.level_lengths())
    return dict(loc=rs.uniform(2.0, 40.0, (B, K, 2)).astype(np.float32),
                conf=rs.normal(0.0, 2.0, (B, K, C)).astype(np.float32),
                prop_loc=rs.normal(0.0, 0.3, (B, K, 2)).astype(np.float32),
                prop_conf=rs.normal(0.0, 2.0, (B, K, C)).astype(np.float32),
                center=rs.normal(0.0, 1.0, (B, K, 1)).astype(np.float32))


def priors():
    return torch.tensor([[(c + 0.5) / t] for t in arch.level_lengths() for c in range(t)], dtype=torch.float32)


@pytest.mark.parametrize("kind", ["focal", "edl"])
def test_closed_set_loss_matches_reference(fx, kind):
    from opental_amd.thumos14.multisegment_loss import MultiSegmentLoss
    crit = MultiSegmentLoss(C, 0.5, 1.0, cls_loss_type=kind, edl_config=EDL_CFG if kind == 'edl' else None, os_head=False)
    ins = {k: torch.from_numpy(v).requires_grad_(True) for k, v in head_outputs().items()}
    targets = [torch.from_numpy(fx["targets_0"]), torch.from_numpy(fx["targets_1"])]
    terms = crit(dict(ins, priors=priors(), act=None, prop_act=None), targets)
    assert terms[5] is None and terms[6] is None
    np.testing.assert_allclose([float(t.detach()) for t in terms[:5]], fx[f"loss_{kind}_terms"], rtol=1e-5)
    sum(float(w) * t for w, t in zip(fx["weights"], terms[:5])).backward()
    for k, v in ins.items():
        ref = fx[f"loss_{kind}_grad_{k}"]
        np.testing.assert_allclose(v.grad.numpy(), ref, rtol=1e-5, atol=1e-5 * float(np.abs(ref).max()), err_msg=k)


@pytest.mark.parametrize("use_edl", [False, True])
def test_get_video_detections_on_closed_set_rows(fx, use_edl):
    """3-column (Softmax) and 4-column (EDL) rows: labels idx_to_class[cl + 1], uncertainty / actionness 0.0 where the
    column is absent -- as the reference's get_video_detections wrote them."""
    from opental_amd.thumos14.test import get_video_detections
    ref = fx[f"dec_edl{int(use_edl)}_fus0_detections"]
    cols = 3 + use_edl
    K, top_k = C - 1, int(fx["decode_params"][1])
    rows = torch.zeros(K, top_k, cols)
    counts = torch.zeros(K, dtype=torch.int32)
    for r in ref:
        cl = int(r[0]) - 1
        rows[cl, counts[cl], :cols] = torch.tensor([r[2], r[3], r[1]] + ([r[4]] if use_edl else []))
        counts[cl] += 1
    idx_to_class = {i: f"class_{i}" for i in range(1, C)}
    props = get_video_detections(rows, counts, idx_to_class, top_k)
    assert len(props) == len(ref)
    got = sorted((p['label'], p['score'], *p['segment'], p['uncertainty'], p['actionness']) for p in props)
    want = sorted((f"class_{int(r[0])}", float(r[1]), float(r[2]), float(r[3]), float(r[4]), float(r[5])) for r in ref)
    assert got == want
    assert all(p['actionness'] == 0.0 for p in props)
    assert all(p['uncertainty'] == 0.0 for p in props) != use_edl


@pytest.fixture(scope="module")
def lib():
    from opental_amd.csrc import build
    if not os.path.exists(build.LIB):
        build.build(verbose=False)
    from opental_amd._lib import declare
    return declare(ctypes.CDLL(build.LIB))


def test_decode_ex_exported_and_checks_arguments(lib):
    assert hasattr(lib, "otal_decode_clips_ex")
    one = ctypes.c_void_p(16)     # never dereferenced: argument checks come first

    def call(loc=one, act=None, prop_act=None, score_fn=1, first_class=1, K=16):
        return lib.otal_decode_clips_ex(loc, one, one, one, one, one, act, prop_act, one, one, one, one, None, None, one,
                                        1, 126, K, 256.0, 0.01, score_fn, first_class, None)
    assert call(loc=None) == -1                       # OTAL_E_NULL
    assert call(act=one) == -1                        # act without prop_act
    assert call(score_fn=2) == -7                     # OTAL_E_UNSUPPORTED
    assert call(score_fn=-1) == -7
    assert call(first_class=2) == -7
    assert call(K=1) == -2                            # nothing left after the background
    # the existing entry keeps its contract: every map present
    assert lib.otal_decode_clips(one, one, one, one, one, one, None, None, one, one, one, one, one, one, one,
                                 1, 126, 16, 256.0, 0.01, None) == -1


def test_softnms_accepts_null_maps_only_where_unread(lib):
    one = ctypes.c_void_p(16)

    def call(unct, actn, cols, nvideos=0):
        return lib.otal_softnms_classes(one, one, unct, actn, one, one, nvideos, 1, 126, 15, 0.5, 10, 0.001, one, one,
                                        None, cols, None)
    # nvideos 0: a shape error comes back once the pointers passed -- i.e. the NULL maps were accepted
    assert call(None, None, 3) == -2
    assert call(one, None, 4) == -2
    assert call(None, None, 4, nvideos=1) == -1
    assert call(one, None, 5, nvideos=1) == -1


def test_loss_modes_check_arguments(lib):
    one = ctypes.c_void_p(16)

    def call(cls_mode, act=one, ibm=0):
        return lib.otal_detection_loss(one, one, one, one, one, act, act, one, one, one, one, 1, 126, C, 1, 256.0, 0.5,
                                       ibm, 50, 0.99, 0, cls_mode, 0.25, one, one, one, None)
    assert call(4) == -7                              # OTAL_E_UNSUPPORTED
    assert call(-1) == -7
    assert call(0, act=None) == -1                    # the OpenTAL modes need the actionness maps
    assert call(1, act=None) == -1
    assert call(2, act=None, ibm=1) == -7             # closed-set EDL: no IBM


def test_out_of_scope_settings_raise():
    from opental_amd.anet.multisegment_loss import MultiSegmentLoss as AnetLoss
    from opental_amd.thumos14.multisegment_loss import MultiSegmentLoss
    from opental_amd.thumos14.test import decode_clips
    with pytest.raises(NotImplementedError):
        MultiSegmentLoss(C, 0.5, 1.0, cls_loss_type='rpl', os_head=False)
    with pytest.raises(NotImplementedError):
        AnetLoss(201, 0.6, 1.0, cls_loss_type='edl', edl_config=dict(EDL_CFG), os_head=False)
    with pytest.raises(NotImplementedError):
        decode_clips({'loc': torch.zeros(1, 126, 2), 'conf': torch.zeros(1, 126, C)}, [0.0], [10.0], os_head=False,
                     use_edl=True, evidence='relu')
