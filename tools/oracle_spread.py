"""Spread of the CPU oracle around the committed forward / ssl vectors (tests/golden/thumos_b1.npz) at a given intra-op
thread count: max |oracle - vector| per output compared by tests/test_oracle_golden.py, and whether the proposal segments
are exact.  Sizes that test's tolerances off the thread count / CPU the vectors were written with (8 threads, Intel
AVX-512).  CPU only.

    python tools/oracle_spread.py [threads ...]        (default: 1 3 8 16)
"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np      # noqa: E402
import torch            # noqa: E402

from oracle import afsd_oracle as O, arch       # noqa: E402

KEYS = ("loc", "conf", "prop_loc", "prop_conf", "center", "act", "prop_act", "unct", "prop_unct")


def spread(fx, P, threads):
    saved = torch.get_num_threads()
    torch.set_num_threads(threads)
    try:
        keep = {}
        with torch.no_grad():
            out = O.bdnet_forward(P, torch.from_numpy(arch.make_clip(int(fx["clip_seed"]), 1)), keep=keep)
        res = {k: float(np.abs(out[k].numpy() - fx["out_" + k]).max()) for k in KEYS}
        res["segments_exact"] = all(np.array_equal(keep["segments"][i].numpy(), fx[f"segments_{i}"]) and
                                    np.array_equal(keep["frame_segments"][i].numpy(), fx[f"frame_segments_{i}"])
                                    for i in range(6))
        x = torch.from_numpy(arch.make_clip(int(fx["ssl_clip_seed"]), 1))
        feat, cost = 0.0, 0.0
        for si in range(fx["ssl_proposals"].shape[0]):
            with torch.no_grad():
                a, p, n = O.ssl_triplets(P, x, [torch.from_numpy(fx["ssl_proposals"][si])])
                c = float(O.triplet_cost(a, p, n, 1.0))
            for nm, got in (("anchor", a), ("positive", p), ("negative", n)):
                for i in range(3):
                    feat = max(feat, float(np.abs(got[i].numpy() - fx[f"ssl{si}_{nm}_{i}"]).max()))
            cost = max(cost, abs(c - float(fx[f"ssl{si}_cost"])))
        res["ssl_features"], res["ssl_cost"] = feat, cost
        return res
    finally:
        torch.set_num_threads(saved)


def main():
    threads = [int(a) for a in sys.argv[1:]] or [1, 3, 8, 16]
    fx = np.load(os.path.join(REPO, "tests", "golden", "thumos_b1.npz"))
    P = O.to_torch(arch.make_params(int(fx["param_seed"])))
    print(f"cpu capability {torch.backends.cpu.get_cpu_capability()}")
    for t in threads:
        r = spread(fx, P, t)
        print(f"threads={t} " + " ".join(f"{k}={v:.2e}" if isinstance(v, float) else f"{k}={v}" for k, v in r.items()),
              flush=True)


if __name__ == "__main__":
    main()
