"""CPU: the anchor-statistics rule (opental_amd/common/anchor_stats.py) against the reference's own numbers
(tests/golden/anchor_stats.npz, written by tools/pin_anchor_stats.py from get_matched_targets, get_result, grad_edl and
plot_grad_density), its refusals, the driver's window selection against get_all_annos on a hand-written annotation list, and
the header's declaration."""
import os

import numpy as np
import pytest
import torch

from anchor_stats_cases import BINS, CASES, case, reference, targets_of

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VALUE_TOL = dict(rtol=1e-5, atol=1e-7)          # the decode kernel's tolerance (tests/test_infer_gpu.py): the same arithmetic


@pytest.fixture(scope="module")
def gold(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "anchor_stats.npz")))


def _rule(gold, target, **kw):
    from opental_amd.common.anchor_stats import anchor_stats_reference
    return anchor_stats_reference(gold['loc'], gold['conf'], gold['prop_conf'], gold['center'], gold['act'], gold['prop_act'],
                                  gold['priors'], gold['gt'], gold['gvalid'], float(gold['clip_length']),
                                  float(gold['overlap_thresh']), True, int(gold['n_known']), target, **kw)


def grad_tolerance(spread, gmax):
    """Four times the reference's own float32-against-float64 spread, no less than the 2e-5 of the ablation tests, of the
    largest |g|."""
    return max(2e-5, 4.0 * float(spread)) * float(gmax)


def test_fixture_is_not_vacuous(gold):
    assert gold['label'].shape == (2, 126, 2) and int(gold['bins']) == BINS
    for s in range(2):
        n = [int((gold['group'][:, :, s] == g).sum()) for g in range(3)]
        assert n[0] >= 10 and n[1] >= 5 and n[2] >= 20, n
    assert (gold['label'][:, :, 0] != gold['label'][:, :, 1]).any()
    assert not (gold['label'][1] > 0).any()                         # sample 1 has no positive anchor
    assert int(gold['label'].max()) > int(gold['n_known'])
    assert float(gold['spread_grad']) < 5e-6                        # so 2e-5 of max |g| is the gradient's tolerance


@pytest.mark.parametrize("target", ['uncertainty', 'actionness', 'confidence', 'uncertainty_actionness', 'half_au'])
def test_rule_against_the_reference(gold, target):
    from opental_amd.common.anchor_stats import TARGETS
    assert tuple(gold['targets']) == TARGETS
    r = _rule(gold, target)
    assert np.array_equal(r['label'], gold['label'])
    assert np.array_equal(r['group'], gold['group'])
    for g in range(3):                                              # the masks of analyze_actionness.py:323-325
        assert np.array_equal(r['group'] == g, gold['group'] == g)
    assert np.array_equal(r['counts'], gold['counts'])
    want = gold['value_' + target]
    print("max |value - reference|", float(np.abs(r['value'] - want).max()))
    np.testing.assert_allclose(r['value'], want, **VALUE_TOL)
    gmax = np.abs(gold['grad']).max()
    print("max |grad - reference| / max |g|", float(np.abs(r['grad'] - gold['grad']).max() / gmax))
    assert np.abs(r['grad'] - gold['grad']).max() <= grad_tolerance(gold['spread_grad'], gmax)
    assert not r['grad'][~gold['counts']].any()                     # rows that do not count hold 0
    assert r['hist_grad'].dtype == np.int64 and np.array_equal(r['hist_grad'], gold['grad_density'])
    for s in range(2):                                              # the score histogram = the reference's values, binned
        for g in range(3):
            v = want[:, :, s][gold['group'][:, :, s] == g]
            bins = np.minimum(np.floor(v.astype(np.float64) * BINS), BINS - 1).astype(np.int64)
            assert np.array_equal(r['hist_score'][s, g], np.bincount(bins, minlength=BINS)), (s, g)


def test_histograms_accumulate_and_host_tensors(gold):
    from opental_amd.common.anchor_stats import anchor_stats
    one = _rule(gold, 'half_au')
    hs, hg = np.full((2, 3, BINS), 5, np.int64), np.full((2, BINS), 7, np.int64)
    _rule(gold, 'half_au', hist_score=hs, hist_grad=hg)
    _rule(gold, 'half_au', hist_score=hs, hist_grad=hg)
    assert np.array_equal(hs, 5 + 2 * one['hist_score']) and np.array_equal(hg, 7 + 2 * one['hist_grad'])
    t = lambda k: torch.from_numpy(gold[k])
    out = dict(hist_score=torch.zeros((2, 3, BINS), dtype=torch.int64), hist_grad=torch.ones((2, BINS), dtype=torch.int64))
    res = anchor_stats(t('loc'), t('conf'), t('prop_conf'), t('center'), t('act'), t('prop_act'), t('priors'), t('gt'),
                       t('gvalid'), 256.0, 0.5, True, 15, 'half_au', out=out)
    assert res['label'].dtype == torch.int32 and res['value'].dtype == torch.float32 and res['grad'].dtype == torch.float32
    assert np.array_equal(res['label'].numpy(), one['label']) and np.array_equal(res['value'].numpy(), one['value'])
    assert np.array_equal(out['hist_score'].numpy(), one['hist_score'])
    assert np.array_equal(out['hist_grad'].numpy(), 1 + one['hist_grad'])


def test_cases_are_usable():
    """make_case asserts its margins and that the THUMOS14 cases are not vacuous; here every committed case is made once."""
    for name in CASES:
        c = case(name)
        assert all(m >= 1e-3 for m in c['margins']), name
    c = case('closed')
    r = reference(c, 'uncertainty')
    assert r['counts'][r['label'] < 16].all() and not r['counts'][r['label'] >= 16].any()   # every anchor has a gradient row
    assert (r['label'] >= 16).any() and r['counts'].sum() > 400
    r = reference(case('few_known'), 'uncertainty')
    assert (r['counts'] & (r['group'] == 1)).any()                  # unknown anchors with a gradient row
    c = case('tie')
    r = reference(c, 'uncertainty')
    tied = (r['area_gap'][0] == 0) & (r['label'][0, :, 0] > 0)
    assert tied.sum() >= 3 and (r['label'][0, tied, 0] == 1).all()  # the first of the two equal areas wins


def test_refusals(gold):
    from opental_amd.common.anchor_stats import ACT_TARGETS, anchor_stats, check_mode
    with pytest.raises(NotImplementedError, match="softmax heads"):
        _rule(gold, 'uncertainty', use_edl=False)
    c = case('closed')
    assert targets_of(c) == ('uncertainty', 'confidence')
    for target in ACT_TARGETS:
        with pytest.raises(NotImplementedError, match="needs the actionness maps"):
            reference(c, target)
        with pytest.raises(NotImplementedError, match="needs the actionness maps"):
            check_mode(target, os_head=False)
        with pytest.raises(NotImplementedError):
            anchor_stats(*[None if c[k] is None else torch.from_numpy(c[k]) for k in
                           ('loc', 'conf', 'prop_conf', 'center', 'act', 'prop_act', 'priors', 'gt', 'gvalid')],
                         256.0, 0.5, False, 15, target)
    with pytest.raises(NotImplementedError):
        _rule(gold, 'a_by_inv_u')
    with pytest.raises(NotImplementedError, match="softmax heads"):
        check_mode('confidence', os_head=False, use_edl=False)


def test_window_selection_follows_get_all_annos():
    """analyze_actionness.py:160-203 on two videos, worked by hand.  'v' (600 sampled frames; windows at 0, 128, 256 and the
    last one at 344): A = [10, 60] lies inside window 0, where B = [200, 300] is cut to [200, 256] (ioa 0.56); B lies inside
    window 128; window 256 sees 43 % of B and 13 % of C = [500, 590] and is dropped; C lies inside window 344.  'w' (100 frames,
    one window): its annotation starts at 0.5, left of the window's first frame 1, so ioa = 39 / 39.5 < 1 and the window is
    dropped although the annotation itself would be kept."""
    from opental_amd.thumos14.analyze_anchors import pad_targets, select_windows
    infos = {'v': {'sample_count': 600}, 'w': {'sample_count': 100}}
    annos = {'v': [[10, 60, 3], [200, 300, 18], [500, 590, 7]], 'w': [[0.5, 40, 2]]}
    got = select_windows(infos, annos, 256, 128)
    assert got == [{'video_name': 'v', 'offset': 0, 'annos': [[10, 60, 3], [200, 256, 18]]},
                   {'video_name': 'v', 'offset': 128, 'annos': [[72, 172, 18]]},
                   {'video_name': 'v', 'offset': 344, 'annos': [[156, 246, 7]]}]
    every = select_windows(infos, annos, 256, 128, all_windows=True)
    assert [(w['video_name'], w['offset']) for w in every] == [('v', 0), ('v', 128), ('v', 256), ('v', 344), ('w', 0)]
    assert every[2]['annos'] == [] and every[4]['annos'] == [] and [w for w in every if w['annos']] == got
    gt, gvalid = pad_targets([w['annos'] for w in every], 256, 'cpu')
    assert tuple(gt.shape) == (5, 2, 3) and gvalid.tolist() == [[1, 1], [1, 0], [0, 0], [1, 0], [0, 0]]
    assert gt[0].tolist() == [[10 / 256, 60 / 256, 3.0], [200 / 256, 1.0, 18.0]]


def test_grad_weights_follow_plot_grad_density(gold):
    from opental_amd.thumos14.analyze_anchors import grad_weights
    for s in range(2):
        np.testing.assert_allclose(grad_weights(gold['grad_density'][s], 0.75), gold['weight_density'][s], rtol=1e-12)


def test_driver_refuses_activitynet():
    from opental_amd.thumos14 import analyze_anchors
    with pytest.raises(NotImplementedError, match="THUMOS14 tool"):
        analyze_anchors.main([os.path.join(REPO, 'configs', 'anet_opental.yaml'), '--open_set', '--split', '0',
                              '--output_npz', 'unused.npz'])


def test_header_declares_the_entry():
    text = open(os.path.join(REPO, 'include', 'opental_hip.h')).read()
    assert 'int otal_anchor_stats(const float* loc, const float* conf, const float* prop_conf' in text
    assert '#define OTAL_ABI_VERSION 26' in text                    # an additive entry
    assert os.path.exists(os.path.join(REPO, 'opental_amd', 'csrc', 'anchorstats.hip'))
