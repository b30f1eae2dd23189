"""The optical-flow training step next to the rgb one, in ONE process on one GPU: python tools/micro_flow_step.py [--batch 8]
[--steps 25] [--runs 7]

Times, at bf16 operands with the ssl branch off (the benchmark's configuration):
  * the resident replayed lane-graph step (inputs already in the captured step's buffers) of the rgb network and of the flow
    network (BDNet(in_channels=2) on zero-plane batches, DESIGN "Training the flow stream");
  * the fed step of each: the same replayed step with ClipStager bringing every batch over PCIe (channels 3 / 2) and the clip
    kernel writing into the captured step's clip buffer;
  * the clip kernels alone at the training shape: otal_prepare_clips (3 channels) and otal_prepare_clips_ch (2 -> 3 planes).
The four step variants ALTERNATE, `--runs` times, `--steps` steps per window after warm-up; a window is a host clock around
work that ends in a device synchronise.  Printed: median and min .. max over the runs (ms per step), clips/s at the median."""
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402
from opental_amd import _lib as L  # noqa: E402
from opental_amd.common import ops, thumos_dataset as D  # noqa: E402
from opental_amd.common.input_pipeline import _PARAM_DTYPE  # noqa: E402

H = W = 112
CLIP, CROP = 256, 96


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def flow_trainer(dev):
    from opental_amd.thumos14.BDNet import BDNet
    from opental_amd.thumos14.multisegment_loss import MultiSegmentLoss
    from opental_amd.thumos14.train import DetectorTrainer
    torch.manual_seed(2020)
    net = BDNet(in_channels=2, training=False, use_edl=True)
    net.backbone._model.apply(BDNet.weight_init)
    net = net.to(dev).train()
    crit = MultiSegmentLoss(15, 0.5, 1.0, cls_loss_type='edl', edl_config=bench.EDL, os_head=True, act_config=bench.ACT).to(dev)
    crit.cls_loss.epoch = 12
    return DetectorTrainer(net, crit, bench.W, lr=1e-5, weight_decay=1e-3)


class Stream:
    """One network with its stager and pre-drawn sample decisions."""

    def __init__(self, name, channels, trainer, batch, dev):
        self.name, self.tr, self.batch = name, trainer, batch
        rs = np.random.RandomState(channels)
        self.videos = [torch.from_numpy(rs.randint(0, 256, (1200, H, W, channels)).astype(np.uint8)).pin_memory() for _ in range(4)]
        self.st = D.ClipStager(batch, CLIP, H, W, CROP, device=dev, max_targets=8, score_rows=2,
                               copy_stream=ops.side_wgrads(dev).side, channels=channels)
        self.pre = [self.samples(300 + k) for k in range(32)]
        self.k = 0
        trainer.launch = 'lanes'

    def samples(self, seed):
        r = np.random.RandomState(seed)
        out = []
        for _ in range(self.batch):
            n = int(r.randint(1, 7))
            a = np.sort(r.uniform(0.0, 1.0, (n, 2)), 1)
            a[:, 1] = np.maximum(a[:, 1], a[:, 0] + 8.0 / CLIP)
            tg = np.concatenate([a, r.randint(1, 16, (n, 1))], 1).astype(np.float32)
            out.append({"video": self.videos[int(r.randint(4))], "offset": int(r.randint(0, 900)), "frame_map": None,
                        "crop": (int(r.randint(17)), int(r.randint(17)), bool(r.randint(2))), "target": tg,
                        "scores": (r.uniform(size=(2, CLIP)) < 0.05).astype(np.float32)})
        return out

    def fed(self, n):
        """n stager-fed steps; leaves no batch pending."""
        st, tr = self.st, self.tr
        st.submit(self.pre[self.k % 32])
        for i in range(n):
            static = tr.static_inputs()
            clips, _ = st.collect(want_ssl=False, out=None if static is None else static[0])
            rec = st.labels()
            self.k += 1
            if i + 1 < n:
                st.submit(self.pre[self.k % 32])
            tr.step(clips, rec.targets, rec.scores)
            st.release()

    def resident(self, n):
        tr = self.tr
        clips, targets, scores = tr.static_inputs()
        for _ in range(n):
            tr.step(clips, targets, scores)


def window(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(n)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def clip_kernels(batch, dev, runs, reps=20):
    """ms per launch of the two clip kernels at the training shape, HIP events around `reps` launches, median over `runs`."""
    lib = L.lib()
    out = torch.empty((batch, 3, CLIP, CROP, CROP), dtype=torch.float32, device=dev)
    res = {}
    for name, c in (("otal_prepare_clips (3 channels)", 3), ("otal_prepare_clips_ch (2 -> 3 planes)", 2)):
        frames = torch.randint(0, 256, (batch * CLIP * H * W * c,), dtype=torch.uint8, device=dev)
        recs = np.zeros(batch, _PARAM_DTYPE)
        for b in range(batch):
            recs[b] = (b * CLIP * H * W * c, CLIP, 3 + b, 5 + b, b & 1)
        params = torch.from_numpy(recs.view(np.uint8).copy()).to(dev)

        def launch():
            if c == 3:
                L.check(lib.otal_prepare_clips(L.ptr(frames), L.ptr(params), L.ptr(out), batch, CLIP, H, W, CROP, CROP, L.stream()),
                        "otal_prepare_clips")
            else:
                L.check(lib.otal_prepare_clips_ch(L.ptr(frames), L.ptr(params), None, L.ptr(out), None, batch, 2, 3, CLIP, H, W,
                                                  CROP, CROP, L.stream()), "otal_prepare_clips_ch")
        for _ in range(5):
            launch()
        ms = []
        for _ in range(runs):
            a, b_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                launch()
            b_.record()
            b_.synchronize()
            ms.append(a.elapsed_time(b_) / reps)
        px = batch * CLIP * CROP * CROP
        res[name] = (ms, px * (c + 12))
    return res


def main():
    batch, steps, runs = arg("--batch", 8), arg("--steps", 25), arg("--runs", 7)
    if not torch.cuda.is_available():
        raise SystemExit("micro_flow_step needs an MI355X")
    dev = torch.device("cuda", 0)
    ops.CONV_PRECISION = 1
    streams = [Stream("rgb", 3, bench.build_trainer(dev), batch, dev), Stream("flow", 2, flow_trainer(dev), batch, dev)]
    for s in streams:
        s.fed(6)                                    # eager step, capture, replays: every shape of the timed windows is warm
        assert s.tr.replayed_steps > 0, s.name + ": the step did not replay"
        s.resident(3)
    variants = [(f"{s.name} {kind}", getattr(s, kind)) for kind in ("resident", "fed") for s in streams]
    times = {name: [] for name, _ in variants}
    for _ in range(runs):
        for name, fn in variants:                   # alternating: drift of the shared host hits every variant alike
            times[name].append(window(fn, steps))
    print(f"b = {batch}, bf16 operands, ssl off, {runs} runs x {steps} steps per variant (ms per step: median, min .. max)")
    for name, _ in variants:
        t = times[name]
        med = statistics.median(t)
        print(f"  {name:14s} {med:8.3f}  {min(t):8.3f} .. {max(t):8.3f}   {batch / med * 1e3:7.0f} clips/s", flush=True)
    for name, (ms, nbytes) in clip_kernels(batch, dev, runs).items():
        med = statistics.median(ms)
        print(f"  {name:40s} {med * 1e3:8.1f} us  {min(ms) * 1e3:8.1f} .. {max(ms) * 1e3:8.1f}   "
              f"{nbytes / med / 1e9:6.2f} TB/s of {nbytes / 1e6:.0f} MB", flush=True)


if __name__ == "__main__":
    main()
