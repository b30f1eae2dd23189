"""tools/pin_closed_set.py -- fixture generator for the closed-set Softmax and EDL baselines (os_head false); runs where the
reference source tree is available, never on the GPU machine.

Imports the reference through oracle.pin_against_reference.import_reference() (as oracle/pin_fusion.py does) and records:
  * loss   -- MultiSegmentLoss(16, 0.5, 1.0, os_head=False) with 'focal' and with 'edl' (configs/thumos14_open_edl.yaml's
              edl_config) on B = 2 synthetic head outputs, C = 16; ragged ground truth, sample 1 without a positive anchor.
              The seven terms (act terms None) and the autograd gradients of cost = sum_i W[i] * term_i with respect to
              loc, conf, prop_loc, prop_conf and center;
  * decode -- parse_output + decode_predictions + filtering + get_video_detections for (use_edl, os_head) = (F, F) and
              (T, F), single-stream (two clips of one video) and fusion (flow "network" = the second sample, as in
              oracle/pin_fusion.py);
  * model  -- the reference BDNet(os_head=False, use_edl=True, training=False) forward at b = 1 with arch.make_params(2020)
              minus the actionness heads and 16-class conf heads drawn from HEAD_SEED (closed_set_params below).

The reference's BDNet.py reads `num_classes` and `os_head` into module globals at import, from the yaml named in
sys.argv (import_reference() names the OpenTAL config: 16 classes, os_head true).  This script sets the module global
`os_head` to False before it builds the model (num_classes is 16 in both configs).

Writes tests/golden/closed_set.npz and tests/golden/PIN_REPORT_closed_set.txt.

    python -m tools.pin_closed_set
"""
import os
import sys

sys.dont_write_bytecode = True
os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
GOLD = os.path.join(REPO, "tests", "golden")

import numpy as np
import torch

from oracle import arch
from oracle.pin_against_reference import REF, import_reference, maxdiff, strided

C = 16
B = 2
LOSS_SEED = 31
HEAD_SEED = 4242
PARAM_SEED = 2020
W = (1.0, 10.0, 1.0, 10.0, 1.0)         # lw, cw, lw, cw, ctw of the THUMOS14 recipe
EDL_CFG = dict(evidence='exp', loss_type='log', soft_label=0, with_focal=False, alpha=0.25, gamma=2)
TARGETS = ([[0.10, 0.30, 3.0], [0.45, 0.62, 7.0], [0.70, 0.95, 15.0]],
           [[0.0, 0.005, 2.0]])             # no prior centre lies in [0, 0.005]: sample 1 has no positive anchor
CLIPS = ((0.0, 10.0), (128.0, 10.0))      # (offset, fps) of the two clips of one video
CONF_THRESH, TOP_K, SIGMA = 0.01, 200, 0.5


def closed_set_params(seed=PARAM_SEED, head_seed=HEAD_SEED):
    """arch.make_params(seed) without the actionness heads, with 16-class conf_head / prop_conf_head (glorot weights, biases
    U(-0.1, 0.1)) from `head_seed`.  Restated in tests/test_closed_set_gpu.py."""
    p = {k: v for k, v in arch.make_params(seed).items() if "actionness_head" not in k}
    rs = np.random.RandomState(head_seed)
    for head, k in (("conf_head", 3), ("prop_conf_head", 1)):
        key = f"coarse_pyramid_detection.{head}.conv1d"
        lim = np.sqrt(3.0 / max(1.0, (512 * k + C * k) / 2.0))
        p[key + ".weight"] = rs.uniform(-lim, lim, size=(C, 512, k)).astype(np.float32)
        p[key + ".bias"] = rs.uniform(-0.1, 0.1, size=(C,)).astype(np.float32)
    return p


def head_outputs():
    """Synthetic (B, 126, .) head outputs: loc / prop_loc in the ranges the network produces, logits of a few units."""
    rs = np.random.RandomState(LOSS_SEED)
    K = sum(arch.level_lengths())
    return dict(loc=rs.uniform(2.0, 40.0, (B, K, 2)).astype(np.float32),
                conf=rs.normal(0.0, 2.0, (B, K, C)).astype(np.float32),
                prop_loc=rs.normal(0.0, 0.3, (B, K, 2)).astype(np.float32),
                prop_conf=rs.normal(0.0, 2.0, (B, K, C)).astype(np.float32),
                center=rs.normal(0.0, 1.0, (B, K, 1)).astype(np.float32))


def priors():
    return torch.tensor([[(c + 0.5) / t] for t in arch.level_lengths() for c in range(t)], dtype=torch.float32)


def pin_loss(MultiSegmentLoss, heads, res, report):
    for kind in ("focal", "edl"):
        crit = MultiSegmentLoss(C, 0.5, 1.0, cls_loss_type=kind, edl_config=EDL_CFG if kind == "edl" else None,
                                os_head=False)
        ins = {k: torch.from_numpy(v.copy()).requires_grad_(True) for k, v in heads.items()}
        out = dict(ins, priors=priors(), act=None, prop_act=None)
        targets = [torch.tensor(t, dtype=torch.float32) for t in TARGETS]
        terms = crit(out, targets)
        assert terms[5] is None and terms[6] is None
        cost = sum(w * t for w, t in zip(W, terms[:5]))
        cost.backward()
        res[f"loss_{kind}_terms"] = np.array([float(t) for t in terms[:5]], np.float64)
        for k, v in ins.items():
            res[f"loss_{kind}_grad_{k}"] = v.grad.numpy().copy()
        report.append(f"loss {kind}: terms {', '.join(f'{float(t):.6f}' for t in terms[:5])}; act terms None")


def outputs_of(heads, i, use_edl):
    """One sample of the synthetic outputs as the reference's network returns them at b = 1."""
    o = {k: torch.from_numpy(v[i:i + 1].copy()) for k, v in heads.items()}
    o["priors"] = priors()
    o["act"] = o["prop_act"] = None
    if use_edl:
        u = lambda z: C / (torch.exp(torch.clamp(z, -10, 10)) + 1).sum(-1)     # DirichletLayer.compute_uncertainty
        o["unct"], o["prop_unct"] = u(o["conf"]), u(o["prop_conf"])
    return o


def pin_decode(ref_test, heads, res, report):
    idx_to_class = {i: f"class_{i}" for i in range(1, C)}
    for use_edl in (False, True):
        score_func = ref_test.DirichletLayer(evidence="exp", dim=-1) if use_edl else torch.nn.Softmax(dim=-1)
        for fusion in (False, True):
            tag = f"dec_edl{int(use_edl)}_fus{int(fusion)}"
            output = [[] for _ in range(C)]
            for ci, (offset, fps) in enumerate(CLIPS):
                rgb = outputs_of(heads, ci if not fusion else 0, use_edl)
                flow = outputs_of(heads, 1, use_edl) if fusion else None
                if fusion and ci == 1:          # second clip of a fused run: swap the two streams
                    rgb, flow = outputs_of(heads, 1, use_edl), outputs_of(heads, 0, use_edl)
                with torch.no_grad():
                    loc, conf, ploc, pconf, center, pri, unct, punct, act, pact = ref_test.parse_output(
                        rgb, flow, fusion=fusion, use_edl=use_edl, os_head=False)
                    seg, score, u, a = ref_test.decode_predictions(
                        loc, ploc, pri, conf, pconf, unct, punct, act, pact, center, offset, fps, 256, C,
                        score_func=score_func, use_edl=use_edl, os_head=False)
                assert a is None and (u is None) == (not use_edl)
                res[f"{tag}_seg_{ci}"] = seg.numpy().copy()
                res[f"{tag}_score_{ci}"] = score.numpy().copy()
                if use_edl:
                    res[f"{tag}_unct_{ci}"] = u.numpy().copy()
                mask = np.zeros((C, seg.shape[0]), np.uint8)
                for cl in range(1, C):
                    mask[cl] = (score[cl] > CONF_THRESH).numpy()
                    rows = ref_test.filtering(seg, score[cl], u, a, CONF_THRESH, use_edl=use_edl, os_head=False)
                    if rows is not None:
                        assert rows.shape[1] == 3 + use_edl
                        output[cl].append(rows)
                res[f"{tag}_mask_{ci}"] = mask
            props = ref_test.get_video_detections(output, idx_to_class, C, TOP_K, SIGMA, use_edl=use_edl, os_head=False,
                                                  cls_rng=range(1, C))
            # rows [class index, score, start, end, uncertainty, actionness] (all float32 values in the reference)
            res[f"{tag}_detections"] = np.array([[float(p['label'].split('_')[1]), p['score'], p['segment'][0],
                                                  p['segment'][1], p['uncertainty'], p['actionness']] for p in props],
                                                np.float32).reshape(-1, 6)
            report.append(f"{tag}: {sum(int(res[f'{tag}_mask_{i}'].sum()) for i in range(2))} rows pass the filter, "
                          f"{len(props)} detections after Soft-NMS")


def pin_model(res, report):
    import AFSD.thumos14.BDNet as ref_bdnet
    ref_bdnet.os_head = False           # see the module docstring
    ref_bdnet.num_classes = C
    net = ref_bdnet.BDNet(training=False, use_edl=True)
    params = closed_set_params()
    sd = net.state_dict()
    assert set(sd) == set(params), sorted(set(sd) ^ set(params))
    net.load_state_dict({k: torch.from_numpy(params[k].copy()) for k in sd})
    net.eval()
    fx = np.load(os.path.join(GOLD, "thumos_b1.npz"))
    seed = int(fx["clip_seed"])
    x = torch.from_numpy(arch.make_clip(seed, 1))
    with torch.no_grad():
        out = net(x)
    assert out["act"] is None and out["conf"].shape == (1, 126, C)
    res["model_clip_seed"] = np.array(seed)
    res["model_param_seed"] = np.array(PARAM_SEED)
    res["model_head_seed"] = np.array(HEAD_SEED)
    for k in ("loc", "conf", "prop_loc", "prop_conf", "center", "unct", "prop_unct"):
        res[f"model_out_{k}"] = out[k].numpy().copy()
    for k in ("start", "end", "start_loc_prop", "end_loc_prop", "start_conf_prop", "end_conf_prop"):
        res[f"model_probe_{k}"] = strided(out[k], 1024)
        res[f"model_sum_{k}"] = np.array(float(out[k].double().sum()))
    report.append(f"model: reference BDNet(os_head=False, use_edl=True) forward at b = 1, clip seed {seed}, "
                  f"params arch.make_params({PARAM_SEED}) - actionness heads + 16-class conf heads (seed {HEAD_SEED})")


def check_against_package(heads, res, report):
    """The package's torch formulation of the closed-set loss on the host, against what was just recorded."""
    from opental_amd.thumos14.multisegment_loss import MultiSegmentLoss
    for kind in ("focal", "edl"):
        crit = MultiSegmentLoss(C, 0.5, 1.0, cls_loss_type=kind, edl_config=EDL_CFG if kind == "edl" else None,
                                os_head=False)
        ins = {k: torch.from_numpy(v.copy()).requires_grad_(True) for k, v in heads.items()}
        terms = crit(dict(ins, priors=priors(), act=None, prop_act=None), [torch.tensor(t) for t in TARGETS])
        sum(w * t for w, t in zip(W, terms[:5])).backward()
        d = max(abs(float(t) - r) for t, r in zip(terms[:5], res[f"loss_{kind}_terms"]))
        g = max(maxdiff(v.grad, torch.from_numpy(res[f"loss_{kind}_grad_{k}"])) for k, v in ins.items())
        report.append(f"loss {kind}: package torch formulation vs reference: max |term diff| {d:.3e}, max |grad diff| {g:.3e}")


def main():
    torch.manual_seed(0)
    _, MultiSegmentLoss, _, _, ref_test = import_reference()
    heads = head_outputs()
    res = {"targets_" + str(i): np.array(t, np.float32) for i, t in enumerate(TARGETS)}
    res["weights"] = np.array(W, np.float64)
    res["clips"] = np.array(CLIPS, np.float64)
    res["decode_params"] = np.array([CONF_THRESH, TOP_K, SIGMA], np.float64)
    report = ["closed-set fixtures (tools/pin_closed_set.py): reference imported with import_reference() (OpenTAL yaml in "
              "sys.argv); BDNet module global os_head set to False before the model is built"]
    pin_loss(MultiSegmentLoss, heads, res, report)
    pin_decode(ref_test, heads, res, report)
    pin_model(res, report)
    check_against_package(heads, res, report)
    np.savez_compressed(os.path.join(GOLD, "closed_set.npz"), **res)
    size = os.path.getsize(os.path.join(GOLD, "closed_set.npz"))
    report.append(f"tests/golden/closed_set.npz: {size} bytes")
    if size >= 300 * 1024:
        import zlib
        big = sorted(((len(zlib.compress(v.tobytes())), k) for k, v in res.items()), reverse=True)[:12]
        raise AssertionError((size, big))
    with open(os.path.join(GOLD, "PIN_REPORT_closed_set.txt"), "w") as f:
        f.write("\n".join(report) + "\n")
    print("\n".join(report))
    leftovers = [os.path.join(d_, n) for d_, _, fs in os.walk(REF) for n in fs if n.endswith(".pyc")]
    assert not leftovers, leftovers


if __name__ == "__main__":
    main()
