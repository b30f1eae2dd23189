"""tools/pin_anet_closed_set.py -- fixture generator for the ActivityNet1.3 closed-set Softmax and EDL baselines (os_head
false); runs where the reference source tree is available, never on the GPU machine, in a process of its own.

Imports the reference's AFSD.anet with configs/anet_edl.yaml in sys.argv: that yaml has no `os_head` key, so the
reference's BDNet.py builds its closed-set globals (num_classes 151, os_head False).  The boundary-pooling op is stubbed
with the CPU oracle as oracle/pin_anet.py does.  Records, with inputs drawn from the seeds below (restated in
tests/test_anet_closed_set_{cpu,gpu}.py, not stored):
  * loss   -- MultiSegmentLoss(151, 0.6, 1.0, os_head=False) with 'focal' and with 'edl' (anet_edl.yaml's edl_config) on
              B = 2 synthetic head outputs (K = 189, priors with level ids); ragged ground truth, sample 1 without a positive
              anchor.  The seven terms (act terms None) and the gradients of cost = sum_i W[i] * term_i with respect to loc,
              conf, prop_loc, prop_conf and center, stored at strided() positions;
  * decode -- decode_prediction + filtering + get_video_prediction of AFSD/anet/test.py for use_edl False (softmax scores)
              and True (Dirichlet scores) on two one-clip videos;
  * model  -- the reference BDNet(use_edl=True, training=False) forward at b = 1 with arch.make_params(2020, arch.ANET)
              minus the actionness heads and 151-class conf heads drawn from HEAD_SEED (closed_set_params below).

Writes tests/golden/anet_closed_set.npz and tests/golden/PIN_REPORT_anet_closed_set.txt.

    python -m tools.pin_anet_closed_set
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

from oracle import afsd_oracle as O
from oracle import arch
from oracle.pin_against_reference import REF, maxdiff, round_margin, strided

CFG = arch.ANET
C = 151
B = 2
PIOU = 0.6
LOSS_SEED = 57
HEAD_SEED = 5151
PARAM_SEED = 2020
CLIP_SEED0 = 30                         # first clip seed tried for the model forward (one with a safe rounding margin is kept)
W = (1.0, 1.0, 1.0, 1.0, 1.0)           # lw, cw, lw, cw, ctw of the ActivityNet recipe (--lw 1 --cw 1)
EDL_CFG = dict(evidence='exp', loss_type='log')              # configs/anet_edl.yaml: training.edl_config
TARGETS = ([[0.10, 0.30, 3.0], [0.45, 0.62, 77.0], [0.70, 0.95, 150.0], [0.05, 0.08, 12.0]],
           [[0.0, 0.005, 2.0]])         # no prior centre lies in [0, 0.005]: sample 1 has no positive anchor
VIDEOS = ((61, 25.0, 29.7), (62, 6.0, 120.0))                 # decode: (head seed, fps, duration in seconds)
CONF_THRESH, TOP_K, SIGMA = 0.001, 5000, 0.85                 # anet/test.py filtering default; configs/anet_*.yaml testing
GRAD_PROBES = 4096


def closed_set_params(seed=PARAM_SEED, head_seed=HEAD_SEED):
    """arch.make_params(seed, ANET) without the actionness heads, with 151-class conf_head / prop_conf_head (glorot weights,
    biases U(-0.1, 0.1)) from `head_seed`.  Restated in tests/test_anet_closed_set_gpu.py."""
    p = {k: v for k, v in arch.make_params(seed, CFG).items() if "actionness_head" not in k}
    rs = np.random.RandomState(head_seed)
    for head, k in (("conf_head", 3), ("prop_conf_head", 1)):
        key = f"coarse_pyramid_detection.{head}.conv1d"
        lim = np.sqrt(3.0 / max(1.0, (512 * k + C * k) / 2.0))
        p[key + ".weight"] = rs.uniform(-lim, lim, size=(C, 512, k)).astype(np.float32)
        p[key + ".bias"] = rs.uniform(-0.1, 0.1, size=(C,)).astype(np.float32)
    return p


def head_outputs(seed=LOSS_SEED, batch=B, center_mean=0.0):
    """Synthetic (batch, 189, .) head outputs in the network's ranges: loc in frames (x the level's stride), logits N(0, 2)."""
    rs = np.random.RandomState(seed)
    pri = O.priors_all(CFG).numpy()
    K = pri.shape[0]
    stride = np.array([CFG["fpn_strides"][int(l)] for l in pri[:, 1]], np.float32)
    return dict(loc=(rs.uniform(0.5, 6.0, (batch, K, 2)) * stride[None, :, None]).astype(np.float32),
                conf=rs.normal(0.0, 2.0, (batch, K, C)).astype(np.float32),
                prop_loc=rs.normal(0.0, 0.3, (batch, K, 2)).astype(np.float32),
                prop_conf=rs.normal(0.0, 2.0, (batch, K, C)).astype(np.float32),
                center=rs.normal(center_mean, 1.0, (batch, K, 1)).astype(np.float32))


def import_reference():
    sys.path.insert(0, REF)
    sys.argv = ["pin", os.path.join(REF, "configs/anet_edl.yaml"), "--open_set", "--split", "0",
                "--lw", "1", "--cw", "1", "--piou", str(PIOU)]
    fake = types.ModuleType("boundary_max_pooling_cuda")
    fake.forward = lambda inp, seg: O.bmp_forward(inp, seg)
    fake.backward = lambda g, inp, seg: O.bmp_backward(g, inp, seg, compat_reference_bwd=True)
    sys.modules["boundary_max_pooling_cuda"] = fake
    torch.Tensor.cuda = lambda self, *a, **k: self
    import AFSD.anet.BDNet as ref_bdnet
    import AFSD.anet.multisegment_loss as ref_loss
    import AFSD.anet.test as ref_test
    from AFSD.common.config import config
    assert ref_bdnet.os_head is False and ref_bdnet.num_classes == C
    assert config['training']['edl_config'] == EDL_CFG, config['training']['edl_config']
    return ref_bdnet, ref_loss, ref_test


def pin_loss(ref_loss, heads, res, report):
    for kind in ("focal", "edl"):
        ref_loss.prior_lb = ref_loss.prior_rb = None
        crit = ref_loss.MultiSegmentLoss(C, PIOU, 1.0, cls_loss_type=kind, edl_config=EDL_CFG if kind == "edl" else None,
                                         os_head=False)
        ins = {k: torch.from_numpy(v.copy()).requires_grad_(True) for k, v in heads.items()}
        pred = [ins["loc"], ins["conf"], ins["prop_loc"], ins["prop_conf"], ins["center"], O.priors_all(CFG), None, None]
        terms = crit(pred, [torch.tensor(t, dtype=torch.float32) for t in TARGETS])
        assert terms[5] is None and terms[6] is None
        sum(w * t for w, t in zip(W, terms[:5])).backward()
        res[f"loss_{kind}_terms"] = np.array([float(t) for t in terms[:5]], np.float64)
        for k, v in ins.items():
            res[f"loss_{kind}_grad_{k}"] = strided(v.grad, GRAD_PROBES)
            res[f"loss_{kind}_gradsum_{k}"] = np.array(float(v.grad.double().abs().sum()))
        report.append(f"loss {kind}: terms {', '.join(f'{float(t):.6f}' for t in terms[:5])}; act terms None")


def pin_decode(ref_test, ref_bdnet, res, report):
    class cfg:
        pass
    cfg.num_classes, cfg.clip_length, cfg.os_head = C, 768, False
    cfg.top_k, cfg.nms_sigma = TOP_K, SIGMA
    cfg.idx_to_class = {i: f"class_{i:03d}" for i in range(1, C)}
    for use_edl in (False, True):
        cfg.use_edl = use_edl
        out_layer = ref_bdnet.DirichletLayer(evidence="exp", dim=-1) if use_edl else torch.nn.Softmax(dim=-1)
        for v, (seed, fps, duration) in enumerate(VIDEOS):
            tag = f"dec_edl{int(use_edl)}_{v}"
            od = {k: torch.from_numpy(a) for k, a in head_outputs(seed, 1, center_mean=-3.0).items()}
            od["priors"] = O.priors_all(CFG)
            if use_edl:
                od["unct"] = out_layer.compute_uncertainty(od["conf"])
                od["prop_unct"] = out_layer.compute_uncertainty(od["prop_conf"])
            with torch.no_grad():
                seg, scores, unct, actn = ref_test.decode_prediction(od, cfg, out_layer)
                assert actn is None and (unct is None) == (not use_edl) and scores.shape[0] == C
                output = [[] for _ in range(C)]
                cls_rng = range(1, C)
                for cl in cls_rng:
                    rows = ref_test.filtering(seg, scores[cl], unct, actn, 0, fps, cfg)
                    if rows is not None:
                        assert rows.shape[1] == 3 + use_edl
                        output[cl].append(rows)
                props = ref_test.get_video_prediction(output, duration, cfg, cls_rng=cls_rng)
            res[f"{tag}_seg"] = seg.numpy().copy()
            res[f"{tag}_score_probe"] = strided(scores[1:], 2048)             # the 150 foreground rows
            res[f"{tag}_nflag"] = np.array(int((scores[1:] > CONF_THRESH).sum()))
            if use_edl:
                res[f"{tag}_unct"] = unct.numpy().copy()
            res[f"{tag}_detections"] = np.array([[float(p['label'].split('_')[1]), p['score'], p['segment'][0],
                                                  p['segment'][1], p['uncertainty'], p['actionness']] for p in props],
                                                np.float32).reshape(-1, 6)
            report.append(f"{tag}: {int(res[f'{tag}_nflag'])} rows pass the filter, {len(props)} detections after "
                          f"Soft-NMS and clipping")


def pin_model(ref_bdnet, res, report):
    net = ref_bdnet.BDNet(training=False, use_edl=True)
    params = closed_set_params()
    sd = net.state_dict()
    assert set(sd) == set(params), sorted(set(sd) ^ set(params))
    net.load_state_dict({k: torch.from_numpy(params[k].copy()) for k in sd})
    net.eval()
    levels = arch.level_lengths(CFG)
    for seed in range(CLIP_SEED0, CLIP_SEED0 + 20):
        x = torch.from_numpy(arch.make_clip(seed, 1, frames=CFG["frame_num"]))
        with torch.no_grad():
            out = net(x)
        margin = round_margin(out["loc"], levels, CFG["frame_num"])
        if margin > 5e-4:
            break
        report.append(f"model: clip seed {seed} skipped (rounding margin {margin:.2e})")
    else:
        raise RuntimeError("no clip seed with a safe rounding margin")
    assert out.get("act") is None and tuple(out["conf"].shape) == (1, 189, C)
    res["model_clip_seed"] = np.array(seed)
    res["model_param_seed"] = np.array(PARAM_SEED)
    res["model_head_seed"] = np.array(HEAD_SEED)
    for k in ("loc", "prop_loc", "center", "unct", "prop_unct"):
        res[f"model_out_{k}"] = out[k].numpy().copy()
    for k in ("conf", "prop_conf"):
        res[f"model_probe_{k}"] = strided(out[k], 4096)
        res[f"model_rowsum_{k}"] = out[k].double().sum(-1).numpy().copy()
    for k in ("start", "end", "start_loc_prop", "end_loc_prop", "start_conf_prop", "end_conf_prop"):
        res[f"model_probe_{k}"] = strided(out[k], 1024)
        res[f"model_sum_{k}"] = np.array(float(out[k].double().sum()))
    report.append(f"model: reference BDNet(use_edl=True, training=False) with os_head False at b = 1, clip seed {seed} "
                  f"(rounding margin {margin:.2e}), params arch.make_params({PARAM_SEED}, ANET) - actionness heads + "
                  f"{C}-class conf heads (seed {HEAD_SEED})")


def check_against_package(heads, res, report):
    """The package's torch formulation of the closed-set loss on the host, against what was just recorded."""
    from opental_amd.anet.multisegment_loss import MultiSegmentLoss
    for kind in ("focal", "edl"):
        crit = MultiSegmentLoss(C, PIOU, 1.0, cls_loss_type=kind, edl_config=EDL_CFG if kind == "edl" else None,
                                os_head=False)
        ins = {k: torch.from_numpy(v.copy()).requires_grad_(True) for k, v in heads.items()}
        terms = crit([ins["loc"], ins["conf"], ins["prop_loc"], ins["prop_conf"], ins["center"], O.priors_all(CFG), None, None],
                     [torch.tensor(t, dtype=torch.float32) for t in TARGETS])
        assert terms[5] is None and terms[6] is None
        sum(w * t for w, t in zip(W, terms[:5])).backward()
        d = max(abs(float(t) - r) for t, r in zip(terms[:5], res[f"loss_{kind}_terms"]))
        g = max(maxdiff(torch.from_numpy(strided(v.grad, GRAD_PROBES)), torch.from_numpy(res[f"loss_{kind}_grad_{k}"]))
                for k, v in ins.items())
        report.append(f"loss {kind}: package torch formulation vs reference: max |term diff| {d:.3e}, "
                      f"max |grad diff| at the probes {g:.3e}")


def main():
    torch.manual_seed(0)
    torch.set_num_threads(os.cpu_count())
    ref_bdnet, ref_loss, ref_test = import_reference()
    heads = head_outputs()
    res = {"targets_" + str(i): np.array(t, np.float32) for i, t in enumerate(TARGETS)}
    res["weights"] = np.array(W, np.float64)
    res["decode_params"] = np.array([CONF_THRESH, TOP_K, SIGMA], np.float64)
    report = ["ActivityNet1.3 closed-set fixtures (tools/pin_anet_closed_set.py): reference AFSD.anet imported with "
              "configs/anet_edl.yaml in sys.argv (no os_head key: closed-set globals, num_classes 151)"]
    pin_loss(ref_loss, heads, res, report)
    check_against_package(heads, res, report)
    pin_decode(ref_test, ref_bdnet, res, report)
    pin_model(ref_bdnet, res, report)
    path = os.path.join(GOLD, "anet_closed_set.npz")
    np.savez_compressed(path, **res)
    size = os.path.getsize(path)
    report.append(f"tests/golden/anet_closed_set.npz: {size} bytes")
    if size >= 300 * 1024:
        import zlib
        big = sorted(((len(zlib.compress(v.tobytes())), k) for k, v in res.items()), reverse=True)[:12]
        raise AssertionError((size, big))
    with open(os.path.join(GOLD, "PIN_REPORT_anet_closed_set.txt"), "w") as f:
        f.write("\n".join(report) + "\n")
    print("\n".join(report))
    leftovers = [os.path.join(d_, n) for d_, _, fs in os.walk(REF) for n in fs if n.endswith(".pyc")]
    assert not leftovers, leftovers


if __name__ == "__main__":
    main()
