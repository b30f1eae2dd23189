#!/bin/bash
# Everything a round commits under profiles/ from ONE box (run through gpurun): kernel statistics on one stream, HBM traffic
# (separate --pmc passes), MFMA utilisation, the per-layer convolution table, the lane-graph step's kernel timeline and the
# default bench line (bench.py --full).   usage: tools/evidence_round.sh r03b DIR   -> DIR/<tag>_*
tag=${1:-rXX}
out=${2:?usage: tools/evidence_round.sh TAG DIR}
bash tools/profile_round.sh $tag "$out"
bash tools/pmc_mfma.sh "$out/${tag}_pmc_mfma_util.txt" > /dev/null 2>&1
OTAL_TOP=400 python tools/profile_convs.py 8 2>/dev/null | grep -v amdgpu.ids > "$out/${tag}_conv_layers_b8_bf16.txt"
bash tools/trace_lanes.sh ${tag}x lanes "$out" > /dev/null 2>&1
mv "$out/${tag}x_step_timeline.txt" "$out/${tag}_step_timeline_lanes.txt"
ls -la "$out/${tag}"_*
