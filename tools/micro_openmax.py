"""Launches the OpenMax kernels and the softmax decode on the same synthetic clips, for kernel-only timing under
`rocprofv3 --kernel-trace --stats` (tools/kernel_time.sh):

    tools/kernel_time.sh 8 -- python tools/micro_openmax.py [clips] [repeats]

32 clips by default: decode_clips_openmax (as shipped and with the refined feature), decode_clips (softmax, os_head False),
class_means and compute_eucos_dist (own class) over the clips' 32 x 126 rows, OpenMax.forward over the same rows."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from opental_amd.thumos14 import test as T, test_openmax as TO
from opental_amd.thumos14.openmax import OpenMax, WeibullFit, class_means, compute_eucos_dist

n = int(sys.argv[1]) if len(sys.argv) > 1 else 32
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 50
K, D, A = 15, 512, 126
dev = torch.device("cuda", 0)
g = torch.Generator().manual_seed(0)
centres = torch.randn(K, D, generator=g).abs()
lab = torch.randint(0, K, (n, A), generator=g)
feat = lambda: (centres[lab] + 0.5 * torch.randn(n, A, D, generator=g)).clamp(min=0).to(dev)
out = dict(loc=(torch.rand(n, A, 2, generator=g) * 30 + 1).to(dev), prop_loc=(torch.randn(n, A, 2, generator=g) * 0.3).to(dev),
           conf=(torch.randn(n, A, K + 1, generator=g) * 2).to(dev), prop_conf=(torch.randn(n, A, K + 1, generator=g) * 2).to(dev),
           center=torch.randn(n, A, 1, generator=g).to(dev), conf_feat=feat(), prop_conf_feat=feat(),
           priors=torch.tensor([[(c + 0.5) / t] for t in (64, 32, 16, 8, 4, 2) for c in range(t)], device=dev))
model = {f"c{k}": {'mean_vec': centres[k].numpy(), 'model': [WeibullFit(10000.08, 2.5e5, 0.12)]} for k in range(K)}
lay = OpenMax(model).to(dev), OpenMax(model).to(dev)
offs, fps = [128.0 * i for i in range(n)], [10.0] * n
rows, labels = out['conf_feat'].reshape(-1, D), lab.reshape(-1).to(dev).int()
for _ in range(reps):
    TO.decode_clips_openmax(out, offs, fps, lay[0], lay[1])
    TO.decode_clips_openmax(out, offs, fps, lay[0], lay[1], refined_feature=True)
    T.decode_clips(out, offs, fps, os_head=False, use_edl=False)
    mav, _ = class_means(rows, labels, K)
    compute_eucos_dist(mav, rows, labels)
    lay[0](out['conf'].reshape(-1, K + 1)[:, 1:], rows)
torch.cuda.synchronize()
print(f"{n} clips, {reps} repeats; decode bytes read once per stage: {n * A * D * 4 / 1e6:.2f} MB of features + {K * D * 4 / 1e3:.1f} KB of MAVs")
