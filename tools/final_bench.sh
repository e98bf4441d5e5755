#!/bin/bash
# the bench line of every workload (headline with --full: the CPU baseline), one JSON line each -> $OUT/final_bench.jsonl
# (a step that fails ends the run: nothing more is started on a GPU that has just faulted or hung)
set -o pipefail
R="$(cd "$(dirname "$0")/.." && pwd)"
cd "$R"
OUT="${OUT:-bench_out}"; mkdir -p "$OUT"
: > "$OUT/final_bench.jsonl"
timeout -k 10 600 python bench.py --steps 20 --warmup 5 --full 2>/dev/null | tail -1 >> "$OUT/final_bench.jsonl" || exit 1
for w in config2 config3 config4 config5; do
  timeout -k 10 600 python bench.py --workload $w --steps 10 --warmup 2 --no-cpu-baseline 2>/dev/null | tail -1 >> "$OUT/final_bench.jsonl" || exit 1
done
python3 - "$OUT/final_bench.jsonl" <<'PY'
import json, sys
for l in open(sys.argv[1]):
    if not l.strip(): continue
    d = json.loads(l)
    print(d["config"].get("name"), "ms/step", d["ms_per_step"], "kernel_ms", d["roofline"]["kernel_ms"], "frac", d["roofline"]["frac"], "value", d["value"], (d.get("cpu_baseline") or {}).get("value"))
PY
