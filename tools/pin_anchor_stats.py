"""tools/pin_anchor_stats.py -- fixture generator for the anchor statistics (opental_amd/common/anchor_stats.py); runs where the
reference source tree is available, never on the GPU machine.

Imports the reference through oracle.pin_against_reference.import_reference() and then its two analysis scripts,
experiments/analyze_actionness.py and experiments/analyze_gradnorm.py (seaborn, which the first imports for its KDE plots, is
replaced by an empty stand-in module; tqdm too where it is missing).  Runs, on B = 2 synthetic head outputs (K = 126, C = 15;
`head_outputs` of tools/pin_ablations.py) with ragged ground truth -- labels on both sides of n_known = 15, sample 1 without a
positive anchor:
  * get_matched_targets (float32 targets, as analyze_gradnorm.py hands them over) -> label (B, K, 2), and the group masks of
    analyze_actionness.py:323-325,:332-334; split_results_by_stages itself is run as a cross-check of the masks;
  * get_result for every target and both stages -> value_<target> (B, K, 2);
  * grad_edl on the rows analyze_gradnorm.py:218-221,:231-234 keep -> grad (B, K, 2), 0 where no row;
  * plot_grad_density (num_bins 100, momentum 0.75) with matplotlib's axes replaced by a recorder -> the grad_density counts
    and the weight curve per stage.

The reference's own rows decide whether a seed is usable.  Every anchor must keep: every score x score_bins at least 1e-3
from an integer (all five targets, both stages); every |g| x grad_bins at least 1e-3 from an integer; every IoU at least
1e-3 from overlap_thresh; the two smallest candidate areas exactly equal or at least 1e-3 frames apart.  The seed is
searched until all four hold, and the margins are printed to the report.

Precision: the same reference code is run once more on float64 inputs; the largest difference of a value, and of a gradient
relative to the largest |g|, is written to the fixture (spread_value, spread_grad) and the report -- the reference's own
float32 error.  The tests allow four times the gradient spread of the largest |g|, and no less than 2e-5.

Writes tests/golden/anchor_stats.npz and tests/golden/PIN_REPORT_anchor_stats.txt.

    python -m tools.pin_anchor_stats
"""
import os
import sys
import types

sys.dont_write_bytecode = True
os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
GOLD = os.path.join(REPO, "tests", "golden")

import numpy as np
import torch

from oracle.pin_against_reference import REF, import_reference
from tools.pin_ablations import head_outputs, priors

B, C, N_KNOWN = 2, 15, 15
CLIP, OVERLAP, BINS, MARGIN = 256, 0.5, 100, 1e-3
TARGETS = ('uncertainty', 'actionness', 'confidence', 'uncertainty_actionness', 'half_au')
# frames of the window, [start, end, label]: labels 3 and 7 are known, 18 and 20 are not; two nested segments (an anchor inside
# both takes the smaller).  No prior centre lies in [0, 1.28]: sample 1 has no positive anchor
ANNOS = ([[25.6, 76.8, 3.0], [115.2, 158.72, 18.0], [179.2, 243.2, 7.0], [190.0, 220.0, 20.0]],
         [[0.0, 1.28, 2.0]])


def import_analysis():
    import_reference()
    for name in ("seaborn", "tqdm"):
        try:
            __import__(name)
        except ImportError:
            sys.modules[name] = types.ModuleType(name)
    import experiments.analyze_actionness as AA
    import experiments.analyze_gradnorm as AG
    from AFSD.thumos14.BDNet import DirichletLayer
    cfg = types.SimpleNamespace(overlap_thresh=OVERLAP, use_edl=True, os_head=True, open_set=True, evidence='exp',
                                num_classes=N_KNOWN, clip_length=CLIP)
    AA.cfg = cfg
    AG.cfg = cfg
    return AA, AG, DirichletLayer


def targets(dtype):
    return [torch.tensor(a, dtype=torch.float64).div(CLIP).mul(torch.tensor([1.0, 1.0, CLIP], dtype=torch.float64)).to(dtype)
            for a in ANNOS]


def run(AA, AG, DirichletLayer, heads, dtype):
    """The reference over the B samples -> dict of (B, K, .) arrays."""
    tdt = torch.float32 if dtype == np.float32 else torch.float64
    h = {k: torch.from_numpy(v.astype(dtype)) for k, v in heads.items()}
    pri = priors().to(tdt)
    tg = targets(tdt)
    loc_t, conf_t, _, prop_conf_t = AA.get_matched_targets(tg, h['loc'], pri, CLIP)
    loc_t2, conf_t2, _, prop_conf_t2 = AG.get_matched_targets(tg, h['loc'], pri, CLIP)        # the same function, copied
    assert torch.equal(conf_t, conf_t2) and torch.equal(prop_conf_t, prop_conf_t2) and torch.equal(loc_t, loc_t2)
    K = pri.shape[0]
    label = torch.stack([conf_t, prop_conf_t], -1).numpy().astype(np.int32)
    out = dict(label=label)
    # the margins' raw material: IoU with the matched target, the two smallest candidate areas
    iou = torch.stack([AA.compute_iou(h['loc'][b], loc_t[b].to(tdt)) for b in range(B)]).numpy()
    gap = np.full((B, K), np.inf)
    for b in range(B):
        t = tg[b]
        left = (pri - t[:, 0][None, :]) * CLIP
        right = (t[:, 1][None, :] - pri) * CLIP
        area = torch.where((left < 0) | (right < 0), torch.full_like(left, 2.0 * CLIP), left + right)
        if area.shape[1] > 1:
            two = torch.sort(area, 1)[0][:, :2]
            gap[b] = (two[:, 1] - two[:, 0]).numpy()
    out.update(iou=iou, area_gap=gap)
    # scores: get_result reads one clip's maps at [0]
    layer = DirichletLayer(evidence='exp', dim=-1)
    for t in TARGETS:
        v = np.zeros((B, K, 2), dtype)
        for b in range(B):
            clip = dict(conf=h['conf'][b:b + 1].numpy(), prop_conf=h['prop_conf'][b:b + 1].numpy(),
                        center=h['center'][b:b + 1].numpy(), act=h['act'][b:b + 1].numpy(),
                        prop_act=h['prop_act'][b:b + 1].numpy(),
                        unct=layer.compute_uncertainty(h['conf'][b:b + 1]).numpy(),
                        prop_unct=layer.compute_uncertainty(h['prop_conf'][b:b + 1]).numpy())
            v[b, :, 0] = AA.get_result(clip, stage='coarse', target=t)
            v[b, :, 1] = AA.get_result(clip, stage='refined', target=t)
        out['value_' + t] = v
    # gradients: analyze_gradnorm.py:214-237 with os_head
    grad = np.zeros((B, K, 2), dtype)
    counts = np.zeros((B, K, 2), bool)
    norms = []
    for s, (logits, lab) in enumerate(((h['conf'], conf_t), (h['prop_conf'], prop_conf_t))):
        conf_p = logits.reshape(-1, C)
        t_conf = lab.reshape(-1, 1)
        keep = (t_conf > 0) & (t_conf <= C)         # a label past the head's columns has no one-hot row (torch.eye(C)[y] fails)
        rows = conf_p[keep.squeeze()]
        y = t_conf[keep].unsqueeze(-1) - 1
        g, gn = AG.grad_edl(rows, y, num_cls=C, evidence='exp')
        flat = np.zeros(B * K, dtype)
        flat[keep.squeeze().numpy()] = g.sum(-1).numpy()
        grad[:, :, s] = flat.reshape(B, K)
        counts[:, :, s] = keep.reshape(B, K).numpy()
        norms.append(gn.numpy())
    out.update(grad=grad, counts=counts, norms=norms)
    return out


class _Axes:
    def __init__(self, rec):
        self.rec = rec

    def plot(self, x, y, *a, **k):
        self.rec.append(np.array(y, dtype=np.float64))

    def twinx(self):
        return _Axes(self.rec)

    def __getattr__(self, name):
        return lambda *a, **k: None


def grad_density(AG, norms):
    """plot_grad_density's grad_density and weight_density, read off what it plots."""
    rec = []
    fake = types.SimpleNamespace(subplots=lambda *a, **k: (None, _Axes(rec)))
    fake.xlabel = fake.xlim = fake.tight_layout = fake.savefig = lambda *a, **k: None
    real, AG.plt = AG.plt, fake
    try:
        AG.plot_grad_density("unused.png", [norms], num_bins=BINS, momentum=0.75)
    finally:
        AG.plt = real
    assert len(rec) == 2
    return rec[0], rec[1]


def margins(r):
    frac = lambda x: float(np.abs(x - np.round(x)).min()) if x.size else np.inf
    m_score = min(frac(r['value_' + t].astype(np.float64) * BINS) for t in TARGETS)
    m_grad = frac(np.abs(r['grad'][r['counts']]).astype(np.float64) * BINS)
    m_iou = float(np.abs(r['iou'].astype(np.float64) - OVERLAP).min())
    gap = r['area_gap'][np.isfinite(r['area_gap']) & (r['area_gap'] != 0)]
    m_area = float(gap.min()) if gap.size else np.inf
    return m_score, m_grad, m_iou, m_area


def main():
    torch.manual_seed(0)
    AA, AG, DirichletLayer = import_analysis()
    report = ["anchor-statistics fixture (tools/pin_anchor_stats.py): reference get_matched_targets, get_result, grad_edl, "
              f"plot_grad_density; B = {B}, K = 126, C = {C}, n_known = {N_KNOWN}, overlap_thresh {OVERLAP}, {BINS} bins",
              f"margins required of every anchor: >= {MARGIN:g}"]
    seed = r32 = None
    for cand in range(31, 20000):
        r = run(AA, AG, DirichletLayer, head_outputs(cand, C, True), np.float32)
        if all(m >= MARGIN for m in margins(r)):
            seed, r32 = cand, r
            break
    assert seed is not None, "no seed meets the margins"
    heads = head_outputs(seed, C, True)
    m = margins(r32)
    report.append(f"head-output seed {seed} (searched from 31)")
    report.append(f"min |score * {BINS} - integer| {m[0]:.4g} (5 targets x 2 stages x {B * 126} anchors); "
                  f"min ||g| * {BINS} - integer| {m[1]:.4g} ({int(r32['counts'].sum())} rows); "
                  f"min |IoU - {OVERLAP}| {m[2]:.4g}; smallest non-zero gap of the two smallest "
                  f"candidate areas {m[3]:.4g} frames")
    label = r32['label']
    group = np.where(label == 0, 2, np.where(label <= N_KNOWN, 0, 1)).astype(np.int32)     # analyze_actionness.py:323-325
    # cross-check of the masks: split_results_by_stages on the same clips (it matches with float64 targets)
    for t in TARGETS:
        tests, annos = [], []
        for b in range(B):
            clip = dict(loc=heads['loc'][b:b + 1], priors=priors().numpy(), conf=heads['conf'][b:b + 1],
                        prop_conf=heads['prop_conf'][b:b + 1], center=heads['center'][b:b + 1], act=heads['act'][b:b + 1],
                        prop_act=heads['prop_act'][b:b + 1],
                        unct=DirichletLayer().compute_uncertainty(torch.from_numpy(heads['conf'][b:b + 1])).numpy(),
                        prop_unct=DirichletLayer().compute_uncertainty(torch.from_numpy(heads['prop_conf'][b:b + 1])).numpy())
            tests.append(dict(name=f"v{b}", offset=[0], rgb_out=[clip]))
            annos.append(dict(video_name=f"v{b}", offset=0, annos=[list(a) for a in ANNOS[b]]))
        known, unknown, bg = AA.split_results_by_stages(tests, annos, target=t)
        for s, stage in enumerate(('coarse', 'refined')):
            for g, parts in enumerate((known, unknown, bg)):
                got = np.concatenate(parts[stage])
                want = r32['value_' + t][:, :, s][group[:, :, s] == g]
                assert np.array_equal(got, want), (t, stage, g)
    counts = [[int((group[:, :, s] == g).sum()) for g in range(3)] for s in range(2)]
    report.append(f"anchors per stage known / unknown / background: coarse {counts[0]}, refined {counts[1]}; "
                  f"{int((label[:, :, 0] != label[:, :, 1]).sum())} anchors lose their label to the IoU test; "
                  f"sample 1: {int((label[1] > 0).sum())} positive anchors")
    dens = [grad_density(AG, n) for n in r32['norms']]
    r64 = run(AA, AG, DirichletLayer, heads, np.float64)
    assert np.array_equal(r64['label'], label)
    sv = max(float(np.abs(r32['value_' + t].astype(np.float64) - r64['value_' + t]).max()) for t in TARGETS)
    gmax = float(np.abs(r64['grad']).max())
    sg = float(np.abs(r32['grad'].astype(np.float64) - r64['grad']).max()) / gmax
    report.append(f"reference float32 vs the same code on float64 inputs: max value diff {sv:.3e}; max grad diff / max |g| "
                  f"{sg:.3e} (max |g| {gmax:.4f}); the tests allow max(2e-5, 4 x that) = {max(2e-5, 4 * sg):.3e} of max |g|")
    G = max(len(a) for a in ANNOS)
    gt = np.zeros((B, G, 3), np.float32)
    gvalid = np.zeros((B, G), np.uint8)
    for b, t in enumerate(targets(torch.float32)):
        gt[b, :len(t)] = t.numpy()
        gvalid[b, :len(t)] = 1
    res = dict(seed=np.array(seed), clip_length=np.array(CLIP), overlap_thresh=np.array(OVERLAP), n_known=np.array(N_KNOWN),
               bins=np.array(BINS), targets=np.array(TARGETS), priors=priors().numpy().reshape(-1), gt=gt, gvalid=gvalid,
               label=label, group=group, grad=r32['grad'], counts=r32['counts'],
               grad_density=np.stack([d[0] for d in dens]).astype(np.int64), weight_density=np.stack([d[1] for d in dens]),
               spread_value=np.array(sv), spread_grad=np.array(sg))
    res.update({k: v.reshape(v.shape[0], v.shape[1], -1).squeeze(-1) if v.shape[-1] == 1 else v for k, v in heads.items()
                if k != 'prop_loc'})
    res.update({'value_' + t: r32['value_' + t] for t in TARGETS})
    report.append(f"grad_density totals: coarse {int(res['grad_density'][0].sum())}, refined {int(res['grad_density'][1].sum())}")
    path = os.path.join(GOLD, "anchor_stats.npz")
    np.savez_compressed(path, **res)
    size = os.path.getsize(path)
    report.append(f"tests/golden/anchor_stats.npz: {size} bytes")
    assert size < 600 * 1024, size
    with open(os.path.join(GOLD, "PIN_REPORT_anchor_stats.txt"), "w") as f:
        f.write("\n".join(report) + "\n")
    print("\n".join(report))
    leftovers = [os.path.join(d_, n) for d_, _, fs in os.walk(REF) for n in fs if n.endswith(".pyc")]
    assert not leftovers, leftovers
    assert not os.path.exists("unused.png")


if __name__ == "__main__":
    main()
