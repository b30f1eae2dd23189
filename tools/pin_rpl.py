"""tools/pin_rpl.py -- fixture generator for the RPL and GCPL baselines (distance head, closed set); runs where the reference
source tree is available, never on the GPU machine.

Imports the reference through oracle.pin_against_reference.import_reference() (as tools/pin_closed_set.py does) and records:
  * head   -- the reference RPLHead forward on seeded (2, 512, 126) features (relu(randn)) and (16, 512) centres, in fp32 and
              in float64, and its autograd backward for a seeded upstream gradient in both precisions.  The float64 distances
              are stored (the float64 gradients are restated by tests/rpl_ref.py, which the report checks against them); of
              the fp32 runs the report keeps the maximum error against float64 (the bound of the GPU tests);
  * loss   -- MultiSegmentLoss(16, 0.5, 1.0, cls_loss_type='rpl', rpl_config=...) for RPL and for GCPL (temperature 1,
              weight_pl 0.1); conf / prop_conf come from the reference RPLHead on the seeded features, loc / prop_loc / center
              and the ragged targets are those of tools/pin_closed_set.py (sample 1 has no positive anchor).  The five terms
              and the autograd gradients of cost = sum_i W[i] * term_i with respect to loc, prop_loc, center, both feature
              maps and both centre tables -- total gradients, with the regulariser's path through feats and centers;
  * decode -- parse_output(use_gcpl=...) + decode_predictions + filtering + get_video_detections for both variants,
              single-stream and fusion, on the distance maps of the loss fixture;
  * model  -- the reference BDNet(use_rpl=True, training=False) forward at b = 1 with arch.make_params(2020) minus the
              actionness and conf-head convolutions, plus the seeded centres.
Feature-sized results are stored as strided probes plus float64 sums; small tensors whole.  The seeds and draws are restated
in tests/rpl_ref.py.  The package's torch formulation is run on the host against what was recorded (report).

Writes tests/golden/rpl.npz and tests/golden/PIN_REPORT_rpl.txt.

    python -m tools.pin_rpl
"""
import os
import sys

sys.dont_write_bytecode = True
os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
GOLD = os.path.join(REPO, "tests", "golden")

import numpy as np
import torch

import rpl_ref as R
from oracle import arch
from oracle.pin_against_reference import REF, import_reference, maxdiff, strided
from tools.pin_closed_set import CLIPS, CONF_THRESH, PARAM_SEED, SIGMA, TARGETS, TOP_K, W, head_outputs, priors

C = R.C
PROBE = 1024
VARIANTS = (("rpl", dict(temperature=1, weight_pl=0.1)), ("gcpl", dict(temperature=1, weight_pl=0.1, gcpl=True)))


def ref_head(RPLHead, centers, dtype):
    h = RPLHead(in_channels=R.D, num_classes=C, num_centers=1)
    h.centers.data = torch.from_numpy(centers.copy()).to(dtype)
    return h


def pin_head(RPLHead, res, report):
    fc, _, cc, _, g = R.seeded_inputs()
    runs = {}
    for dtype in (torch.float32, torch.float64):
        h = ref_head(RPLHead, cc, dtype)
        x = torch.from_numpy(fc.copy()).to(dtype).requires_grad_(True)
        dist = h(x)
        (dist * torch.from_numpy(g.copy()).to(dtype)).sum().backward()
        runs[dtype] = (dist.detach(), x.grad.clone(), h.centers.grad.clone())
    d32, dx32, dc32 = runs[torch.float32]
    d64, dx64, dc64 = runs[torch.float64]
    res["head_dist_f64"] = d64.numpy().copy()
    errs = (maxdiff(d32, d64), maxdiff(dx32, dx64), maxdiff(dc32, dc64))
    res["head_ref_fp32_err"] = np.array(errs, np.float64)
    report.append(f"head: reference RPLHead fp32 vs float64: max |dist err| {errs[0]:.6e}, max |dx err| {errs[1]:.6e}, "
                  f"max |dcenters err| {errs[2]:.6e} (max |dist| {float(d64.abs().max()):.4f}, "
                  f"max |dx| {float(dx64.abs().max()):.4e}, max |dcenters| {float(dc64.abs().max()):.4e})")
    own = R.head_fwd(fc, cc)
    odx, odc = R.head_bwd(fc, cc, g)
    report.append(f"head: tests/rpl_ref.py float64 vs the reference's float64: dist {np.abs(own - d64.numpy()).max():.3e}, "
                  f"dx {np.abs(odx - dx64.numpy()).max():.3e}, dcenters {np.abs(odc - dc64.numpy()).max():.3e}")


def loss_inputs(RPLHead):
    """Leaves and the reference's output dict of the loss fixture."""
    fc, fp, cc, cp, _ = R.seeded_inputs()
    heads = head_outputs()
    ins = {k: torch.from_numpy(heads[k].copy()).requires_grad_(True) for k in ("loc", "prop_loc", "center")}
    ins["feat"] = torch.from_numpy(fc.copy()).requires_grad_(True)
    ins["prop_feat"] = torch.from_numpy(fp.copy()).requires_grad_(True)
    hc, hp = ref_head(RPLHead, cc, torch.float32), ref_head(RPLHead, cp, torch.float32)
    ins["centers"], ins["prop_centers"] = hc.centers, hp.centers
    tr = lambda y: y.permute(0, 2, 1).contiguous()
    out = dict(loc=ins["loc"], prop_loc=ins["prop_loc"], center=ins["center"], priors=priors(), act=None, prop_act=None,
               conf=tr(hc(ins["feat"])), prop_conf=tr(hp(ins["prop_feat"])), cls_ctr=hc.centers, prop_cls_ctr=hp.centers,
               ctr_feat=tr(ins["feat"]), prop_ctr_feat=tr(ins["prop_feat"]))
    return ins, out


def store_grads(res, tag, ins):
    for k, v in ins.items():
        g = v.grad
        if k in ("feat", "prop_feat"):
            res[f"{tag}_grad_{k}_probe"] = strided(g, PROBE)
            res[f"{tag}_grad_{k}_sum"] = np.array(float(g.double().sum()))
            res[f"{tag}_grad_{k}_abssum"] = np.array(float(g.double().abs().sum()))
        else:
            res[f"{tag}_grad_{k}"] = g.numpy().copy()


def pin_loss(MultiSegmentLoss, RPLHead, res, report):
    for name, cfg in VARIANTS:
        crit = MultiSegmentLoss(C, 0.5, 1.0, cls_loss_type='rpl', rpl_config=dict(cfg))
        ins, out = loss_inputs(RPLHead)
        terms = crit(out, [torch.tensor(t, dtype=torch.float32) for t in TARGETS])
        assert terms[5] is None and terms[6] is None
        sum(w * t for w, t in zip(W, terms[:5])).backward()
        res[f"loss_{name}_terms"] = np.array([float(t) for t in terms[:5]], np.float64)
        store_grads(res, f"loss_{name}", ins)
        report.append(f"loss {name}: terms {', '.join(f'{float(t):.6f}' for t in terms[:5])}; act terms None")


def pin_decode(ref_test, RPLHead, res, report):
    idx_to_class = {i: f"class_{i}" for i in range(1, C)}
    heads = head_outputs()
    fc, fp, cc, cp, _ = R.seeded_inputs()
    with torch.no_grad():               # the distance maps of the loss fixture: the reference head in fp32
        for k, f, c in (("conf", fc, cc), ("prop_conf", fp, cp)):
            heads[k] = ref_head(RPLHead, c, torch.float32)(torch.from_numpy(f.copy())).permute(0, 2, 1).contiguous().numpy()

    def outputs_of(i):
        o = {k: torch.from_numpy(v[i:i + 1].copy()) for k, v in heads.items()}
        o["priors"] = priors()
        o["act"] = o["prop_act"] = None
        return o
    for name, cfg in VARIANTS:
        gcpl = bool(cfg.get("gcpl", False))
        for fusion in (False, True):
            tag = f"dec_{name}_fus{int(fusion)}"
            output = [[] for _ in range(C)]
            passed = 0
            for ci, (offset, fps) in enumerate(CLIPS):
                rgb, flow = outputs_of(ci if not fusion else 0), (outputs_of(1) if fusion else None)
                if fusion and ci == 1:          # second clip of a fused run: swap the two streams
                    rgb, flow = outputs_of(1), outputs_of(0)
                with torch.no_grad():
                    loc, conf, ploc, pconf, center, pri, unct, punct, act, pact = ref_test.parse_output(
                        rgb, flow, fusion=fusion, use_edl=False, os_head=False, use_gcpl=gcpl)
                    seg, score, u, a = ref_test.decode_predictions(
                        loc, ploc, pri, conf, pconf, unct, punct, act, pact, center, offset, fps, 256, C,
                        score_func=torch.nn.Softmax(dim=-1), use_edl=False, os_head=False)
                assert a is None and u is None
                res[f"{tag}_seg_{ci}"] = seg.numpy().copy()
                res[f"{tag}_score_{ci}"] = score.numpy().copy()
                for cl in range(1, C):
                    rows = ref_test.filtering(seg, score[cl], u, a, CONF_THRESH, use_edl=False, os_head=False)
                    if rows is not None:
                        passed += rows.shape[0]
                        output[cl].append(rows)
            props = ref_test.get_video_detections(output, idx_to_class, C, TOP_K, SIGMA, use_edl=False, os_head=False,
                                                  cls_rng=range(1, C))
            res[f"{tag}_detections"] = np.array([[float(p['label'].split('_')[1]), p['score'], p['segment'][0],
                                                  p['segment'][1], p['uncertainty'], p['actionness']] for p in props],
                                                np.float32).reshape(-1, 6)
            report.append(f"{tag}: {passed} rows pass the filter, {len(props)} detections after Soft-NMS")


def rpl_params(seed=PARAM_SEED):
    """arch.make_params(seed) without the actionness and conf-head convolutions, plus the seeded centres of tests/rpl_ref.py.
    Restated in tests/test_rpl_gpu.py."""
    p = {k: v for k, v in arch.make_params(seed).items()
         if "actionness_head" not in k and ".conf_head." not in k and ".prop_conf_head." not in k}
    _, _, cc, cp, _ = R.seeded_inputs()
    p["coarse_pyramid_detection.conf_head.centers"] = cc
    p["coarse_pyramid_detection.prop_conf_head.centers"] = cp
    return p


def pin_model(res, report):
    import AFSD.thumos14.BDNet as ref_bdnet
    ref_bdnet.os_head = False           # module globals read from the OpenTAL yaml at import (see tools/pin_closed_set.py)
    ref_bdnet.num_classes = C
    net = ref_bdnet.BDNet(training=False, use_rpl=True)
    params = rpl_params()
    sd = net.state_dict()
    assert set(sd) == set(params), sorted(set(sd) ^ set(params))
    net.load_state_dict({k: torch.from_numpy(params[k].copy()) for k in sd})
    net.eval()
    seed = int(np.load(os.path.join(GOLD, "thumos_b1.npz"))["clip_seed"])
    with torch.no_grad():
        out = net(torch.from_numpy(arch.make_clip(seed, 1)))
    assert out["act"] is None and out["conf"].shape == (1, 126, C) and "cls_ctr" not in out
    res["model_clip_seed"] = np.array(seed)
    for k in ("loc", "conf", "prop_loc", "prop_conf", "center"):
        res[f"model_out_{k}"] = out[k].numpy().copy()
    report.append(f"model: reference BDNet(use_rpl=True, training=False) forward at b = 1, clip seed {seed}, params "
                  f"arch.make_params({PARAM_SEED}) - actionness / conf-head convolutions + seeded centres; conf in "
                  f"[{float(out['conf'].min()):.4f}, {float(out['conf'].max()):.4f}]")


def check_against_package(res, report):
    """The package's torch formulation (RPLHead and MultiSegmentLoss on host tensors) against what was just recorded."""
    from opental_amd.common.layers import RPLHead
    from opental_amd.thumos14.multisegment_loss import MultiSegmentLoss
    for name, cfg in VARIANTS:
        crit = MultiSegmentLoss(C, 0.5, 1.0, cls_loss_type='rpl', rpl_config=dict(cfg))
        ins, out = loss_inputs(RPLHead)
        terms = crit(out, [torch.tensor(t) for t in TARGETS])
        sum(w * t for w, t in zip(W, terms[:5])).backward()
        d = max(abs(float(t) - r) for t, r in zip(terms[:5], res[f"loss_{name}_terms"]))
        g = 0.0
        for k, v in ins.items():
            if k in ("feat", "prop_feat"):
                g = max(g, float(np.abs(strided(v.grad, PROBE) - res[f"loss_{name}_grad_{k}_probe"]).max()))
            else:
                g = max(g, maxdiff(v.grad, torch.from_numpy(res[f"loss_{name}_grad_{k}"])))
        report.append(f"loss {name}: package torch formulation vs reference: max |term diff| {d:.3e}, max |grad diff| {g:.3e}")


def main():
    torch.manual_seed(0)
    _, MultiSegmentLoss, _, _, ref_test = import_reference()
    from AFSD.common.layers import RPLHead
    res = {"targets_" + str(i): np.array(t, np.float32) for i, t in enumerate(TARGETS)}
    res["weights"] = np.array(W, np.float64)
    res["clips"] = np.array(CLIPS, np.float64)
    res["decode_params"] = np.array([CONF_THRESH, TOP_K, SIGMA], np.float64)
    report = ["RPL / GCPL fixtures (tools/pin_rpl.py): reference imported with import_reference() (OpenTAL yaml in sys.argv); "
              "BDNet module global os_head set to False before the model is built"]
    pin_head(RPLHead, res, report)
    pin_loss(MultiSegmentLoss, RPLHead, res, report)
    pin_decode(ref_test, RPLHead, res, report)
    pin_model(res, report)
    check_against_package(res, report)
    path = os.path.join(GOLD, "rpl.npz")
    np.savez_compressed(path, **res)
    size = os.path.getsize(path)
    report.append(f"tests/golden/rpl.npz: {size} bytes")
    if size >= 300 * 1024:
        import zlib
        big = sorted(((len(zlib.compress(v.tobytes())), k) for k, v in res.items()), reverse=True)[:12]
        raise AssertionError((size, big))
    with open(os.path.join(GOLD, "PIN_REPORT_rpl.txt"), "w") as f:
        f.write("\n".join(report) + "\n")
    print("\n".join(report))
    leftovers = [os.path.join(d_, n) for d_, _, fs in os.walk(REF) for n in fs if n.endswith(".pyc")]
    assert not leftovers, leftovers


if __name__ == "__main__":
    main()
