O=$(realpath -m "${1:?usage: $0 OUTPUT_DIR}"); mkdir -p "$O"
cd /root/repo
T0=$(date +%s)
python bench.py --full --gpus 1 --steps 20 --warmup 5 > $O/r4_bench_b.json 2> $O/r4_bench_b.err
echo "bench wall $(( $(date +%s) - T0 )) s"
grep -E "Error|error|Traceback" $O/r4_bench_b.err | head
python - <<PY
import json
d=json.load(open("$O/r4_bench_b.json"))
print(d["value"], d["ms_per_step"], d["power"], d["steady_state"])
print(d["cpu_baseline"])
for k,v in d["configs"].items(): print(k, {kk: v.get(kk) for kk in ("value","ms_per_step","steps","error","power")}, (v.get("roofline") or {}).get("frac_algorithmic"))
print(d["roofline"]["by_kernel_ms_per_step"])
PY
