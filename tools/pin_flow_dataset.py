"""tools/pin_flow_dataset.py -- writes tests/golden/flow_dataset.npz; needs a checkout of the reference (imported at run
time, never copied): python tools/pin_flow_dataset.py <path to the reference checkout>

The optical-flow stream's dataset fixture.  The reference's THUMOS_Dataset.__getitem__ (AFSD/common/thumos_dataset.py:
239-275) runs on the seeded synthetic 2-channel dataset of tests/flow_cases.py -- frames (300,12,14,2), clip_length 32,
crop_size 8, two annotations, a second video shorter than a clip -- for four (sample, seed) pairs chosen so that one is
flipped, one has a successful ssl splice and one window is shorter than the clip.  Written: the frames, the seeds, and per
sample the decisions (this repository's THUMOS_Dataset.decide under the same seed, asserted equal to what the reference's
pixels imply), the reference's clip and ssl clip (2,32,8,8) fp32, and the targets.
tests/test_flow_cpu.py checks the decisions, tests/test_flow_gpu.py the pixels (ClipStager(channels=2))."""
import os
import random
import sys
import types

sys.dont_write_bytecode = True
os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np
import torch

import flow_cases as F


def main(ref):
    sys.path.insert(0, ref)
    sys.argv = ["pin", os.path.join(ref, "configs/thumos14_opental_final.yaml"), "--open_set", "--split", "0"]
    fake = types.ModuleType("boundary_max_pooling_cuda")
    fake.forward = fake.backward = None
    sys.modules["boundary_max_pooling_cuda"] = fake
    import AFSD.common.thumos_dataset as RD
    from opental_amd.common import thumos_dataset as MD

    frames = F.make_frames()
    infos, annos, videos = F.dataset_tables(frames)
    r_data = {n: np.transpose(v, [3, 0, 1, 2]) for n, v in videos.items()}          # load_video_data's layout, :136-137
    m_data = {n: torch.from_numpy(v) for n, v in videos.items()}
    r_ds = RD.THUMOS_Dataset(r_data, infos, annos, clip_length=F.CLIP, crop_size=F.CROP, stride=F.STRIDE)
    m_ds = MD.THUMOS_Dataset(m_data, infos, annos, clip_length=F.CLIP, crop_size=F.CROP, stride=F.STRIDE)
    assert len(r_ds) == len(m_ds) >= 3
    for a, b in zip(r_ds.training_list, m_ds.training_list):
        assert a['video_name'] == b['video_name'] and a['offset'] == b['offset'] and a['annos'] == b['annos']

    def draw(idx, seed):
        random.seed(seed)
        x, target, scores, ssl_x, ssl_target, flag = r_ds[idx]
        random.seed(seed)
        d = m_ds.decide(idx)
        assert bool(flag) == bool(d['flag'])
        assert np.allclose(np.asarray(target, np.float32), d['target']) and np.array_equal(scores.numpy(), d['scores'])
        assert np.array_equal(np.asarray(ssl_target, np.float32), d['ssl_target'])
        return d, x.numpy(), ssl_x.numpy()

    short = [i for i, s in enumerate(m_ds.training_list) if s['video_name'] == "flow_short"]
    long_ = [i for i, s in enumerate(m_ds.training_list) if s['video_name'] == "flow_long"]
    assert short and long_

    def first(indices, want):
        for seed in range(200):
            for idx in indices:
                d, _, _ = draw(idx, seed)
                if want(d):
                    return idx, seed
        raise AssertionError("no (sample, seed) with the wanted decisions")
    picks = [first(short, lambda d: True),                                     # a window shorter than the clip
             first(long_, lambda d: d['crop'][2] and not d['flag']),           # flipped
             first(long_, lambda d: d['flag'] and not d['crop'][2]),           # a successful ssl splice
             first(long_, lambda d: d['flag'] and d['crop'][2])]               # both
    fx = {"frames": frames, "picks": np.asarray(picks, np.int64)}
    for k, (idx, seed) in enumerate(picks):
        d, clip, ssl_clip = draw(idx, seed)
        assert clip.shape == ssl_clip.shape == (2, F.CLIP, F.CROP, F.CROP) and clip.dtype == np.float32
        i, j, flip = d['crop']
        valid = min(F.CLIP, videos[m_ds.training_list[idx]['video_name']].shape[0] - d['offset'])
        fx[f"decision_{k}"] = np.array([i, j, int(flip), d['offset'], int(d['flag']), valid], np.int64)
        fx[f"map_{k}"] = d['frame_map'] if d['frame_map'] is not None else np.zeros(0, np.int32)
        fx[f"clip_{k}"], fx[f"ssl_clip_{k}"] = clip, ssl_clip
        fx[f"target_{k}"], fx[f"ssl_target_{k}"] = d['target'], d['ssl_target']
    assert fx["decision_0"][5] < F.CLIP
    out = os.path.join(REPO, "tests", "golden", "flow_dataset.npz")
    np.savez_compressed(out, **fx)
    print(f"wrote {out}: {os.path.getsize(out)} bytes, picks {picks}")
    leftovers = [os.path.join(d_, n) for d_, _, fs in os.walk(ref) for n in fs if n.endswith(".pyc")]
    assert not leftovers, leftovers


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
