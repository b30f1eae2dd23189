"""The synthetic 2-channel dataset behind tests/golden/flow_dataset.npz, shared by the tool that writes the fixture
(tools/pin_flow_dataset.py, which runs the reference's THUMOS_Dataset.__getitem__ on it) and the tests that read it
(test_flow_cpu.py: the decisions; test_flow_gpu.py: the pixels).  The fixture holds the frames; the two videos are cut from
them here, the second one shorter than a clip."""
import numpy as np

CLIP, CROP, STRIDE = 32, 8, 16
FRAMES_SHAPE = (300, 12, 14, 2)
FRAMES_SEED = 77
SHORT = 20                                  # frames of the short video: the first SHORT frames of the long one
# two annotations, in sampled frames: [start, end, class]; the short video only sees the first
ANNOS = [[6.0, 10.0, 1], [150.0, 162.0, 2]]


def make_frames():
    return np.random.RandomState(FRAMES_SEED).randint(0, 256, FRAMES_SHAPE).astype(np.uint8)


def dataset_tables(frames):
    """(video_infos, video_annos, videos) in the form THUMOS_Dataset takes them; videos are (T,H,W,2) uint8."""
    videos = {"flow_long": frames, "flow_short": np.ascontiguousarray(frames[:SHORT])}
    infos = {n: {"fps": 30.0, "sample_fps": 10.0, "count": 3 * v.shape[0], "sample_count": int(v.shape[0])}
             for n, v in videos.items()}
    annos = {"flow_long": [list(a) for a in ANNOS], "flow_short": [list(ANNOS[0])]}
    return infos, annos, videos
