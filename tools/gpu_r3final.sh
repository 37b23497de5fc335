#!/bin/bash
# round 3, final binary: every tracked profile re-collected (bench default, configs[3], configs[2], training step, generic unit
# steps), then the default bench line with every secondary block (--full) into the directory given as $1
set -o pipefail
O=${1:?usage: tools/gpu_r3final.sh <output directory>}; mkdir -p "$O"
bash tools/collect_profiles.sh r03 || exit 1
bash tools/collect_profiles.sh r03_cfg3 --frames 200 --graph LMDHG || exit 1
bash tools/collect_profiles.sh r03_cfg2 --clips-per-gpu 512 --frames 500 || exit 1
bash tools/collect_counters.sh r03_train tools/train_step.py --steps 20 --warmup 5 || exit 1
bash tools/collect_counters.sh r03_generic tools/generic_unit_step.py --steps 10 || exit 1
timeout -k 10 300 python bench.py --full > "$O/r03_final_bench.json" 2> "$O/r03_final_bench.err" || { tail -5 "$O/r03_final_bench.err"; exit 1; }
tail -c 600 "$O/r03_final_bench.json"
