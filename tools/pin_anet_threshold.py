"""tools/pin_anet_threshold.py -- pins the one pure function of the reference's ActivityNet thresholding script; runs on the
CPU where the reference source tree is available, never on the GPU machine.

AFSD/anet/threshold.py cannot be imported whole (it imports a `test` module from the working directory and, as shipped, calls
inference_thread with one argument too many), so only `compute_threshold` (:13-28) is taken out of it: the file is parsed,
that one function definition is compiled and run here, with numpy as its only global.  Nothing of the reference is written
into the repository; the golden file holds the inputs and the numbers the function returned.

Inputs: seeded synthetic result dicts (videos -> proposal lists with 'score', 'uncertainty', 'actionness' holding float32
values, as the drivers' dicts do) of 1, 20, 137 and 1000 detections, for the reference's three scorings.

Writes tests/golden/anet_threshold.npz (per case `n<N>_video`, `n<N>_sup` (N, 3) float32 = score, uncertainty, actionness,
`n<N>_threshold` (3,) float64 in the order of `scorings`) and tests/golden/PIN_REPORT_anet_threshold.txt.

    python -m tools.pin_anet_threshold
"""
import ast
import os
import sys

sys.dont_write_bytecode = True
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
GOLD = os.path.join(REPO, "tests", "golden")

import numpy as np

SCORINGS = ("uncertainty", "confidence", "uncertainty_actionness")      # the three branches of compute_threshold
CASES = (1, 20, 137, 1000)
SEED = 20261018


def reference_compute_threshold(ref_root):
    path = os.path.join(ref_root, "AFSD", "anet", "threshold.py")
    with open(path) as f:
        tree = ast.parse(f.read(), path)
    node = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "compute_threshold")
    scope = {"np": np}
    exec(compile(ast.Module(body=[node], type_ignores=[]), path, "exec"), scope)
    return scope["compute_threshold"]


def synthetic(n, rs):
    """-> video (n,) int32 ascending over 3 videos, sup (n, 3) float32 = score, uncertainty, actionness in (0, 1)."""
    video = np.sort(rs.randint(0, 3, n)).astype(np.int32)
    sup = rs.uniform(0.02, 0.98, (n, 3)).astype(np.float32)
    return video, sup


def result_dict(video, sup):
    out = {f"video_{v}": [] for v in range(3)}
    for v, (s, u, a) in zip(video.tolist(), sup.astype(np.float64).tolist()):
        out[f"video_{v}"].append({"label": 1, "score": s, "segment": [0.0, 1.0], "uncertainty": u, "actionness": a})
    return out


def main():
    from oracle.pin_against_reference import REF
    compute_threshold = reference_compute_threshold(REF)
    rs = np.random.RandomState(SEED)
    out, lines = {"scorings": np.array(SCORINGS)}, ["compute_threshold of the reference's anet/threshold.py on synthetic dicts", ""]
    for n in CASES:
        video, sup = synthetic(n, rs)
        thr = np.array([float(compute_threshold(result_dict(video, sup), scoring=s)) for s in SCORINGS], dtype=np.float64)
        out[f"n{n}_video"], out[f"n{n}_sup"], out[f"n{n}_threshold"] = video, sup, thr
        lines.append(f"N = {n:5d}  position {n - int(n * 0.95) - 1:3d}  " +
                     "  ".join(f"{s} {t:.17g}" for s, t in zip(SCORINGS, thr)))
    np.savez(os.path.join(GOLD, "anet_threshold.npz"), **out)
    with open(os.path.join(GOLD, "PIN_REPORT_anet_threshold.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
