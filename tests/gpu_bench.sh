#!/bin/bash
# GPU box: smoke, bench (headline), rocprofv3 kernel trace of the same command
set -e
R="$(cd "$(dirname "$0")/.." && pwd)"
cd "$R"
OUT="$(mkdir -p "${OUT:-bench_out}" && cd "${OUT:-bench_out}" && pwd)"
make -s -C oracle _build/libeu_oracle.so
python __graft_entry__.py smoke 2>&1 | tee "$OUT/smoke.log"
python bench.py --workload small --steps 5 --warmup 1 --full 2>&1 | tee "$OUT/bench_small.log"
python bench.py --steps 20 --warmup 3 --full 2>&1 | tee "$OUT/bench_headline.log"
export TMPDIR=/tmp
cd /tmp
rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof_headline" -- python3 "$R/bench.py" --steps 10 --warmup 2 --no-cpu-baseline > "$OUT/prof_headline.log" 2>&1
cd "$R"
find "$OUT/prof_headline" -name "*stats*" | head
