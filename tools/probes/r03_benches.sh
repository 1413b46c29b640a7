#!/bin/bash
# the round's bench lines on one box: headline shape, configs[1], SISR, training steps, + the 64-channel wx4 experiment
O=$(realpath -m "${1:?usage: $0 OUTPUT_DIR}"); mkdir -p "$O"
cd /root/repo
python bench.py --full --steps 20 --warmup 5 > $O/r03_bench_256.json 2> $O/r03_bench_256.err
VIRNET_WX4_MIN_COUT=64 python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline > $O/r03_bench_256_wx64.json 2>/dev/null
python bench.py --full --size 128 --batch 64 --steps 20 --warmup 5 --no-cpu-baseline > $O/r03_bench_128.json 2>/dev/null
python bench.py --full --task sisr --steps 20 --warmup 5 > $O/r03_bench_sisr.json 2>/dev/null
python bench.py --full --task train --steps 10 --warmup 3 > $O/r03_bench_train.json 2>/dev/null
python bench.py --full --task train --dtype bf16 --steps 10 --warmup 3 > $O/r03_bench_train_bf16.json 2>/dev/null
python bench.py --full --task train_sisr --steps 10 --warmup 3 > $O/r03_bench_train_sisr.json 2>/dev/null
for f in 256 256_wx64 128 sisr train train_bf16 train_sisr; do python - <<PY
import json
try:
    d=json.load(open("$O/r03_bench_$f.json")); print("$f", d["value"], d["ms_per_step"], d.get("roofline",{}).get("by_kernel_ms_per_step"))
except Exception as e: print("$f FAILED", e)
PY
done
{ echo "# wx4 (default)"; python tools/bench_latency.py; python tools/bench_latency.py --graph; echo "# VIRNET_CONV_FORM=f16x3 (round 2's kernels)"; VIRNET_CONV_FORM=f16x3 python tools/bench_latency.py; } 2>/dev/null | grep -v amdgpu > $O/r03_latency.txt
cat $O/r03_latency.txt
