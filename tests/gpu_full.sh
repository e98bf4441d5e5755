#!/bin/bash
# full GPU pass: all gpu tests, smoke, headline bench + rocprofv3 kernel trace of the same command
set -e
R="$(cd "$(dirname "$0")/.." && pwd)"; cd "$R"
OUT="$(mkdir -p "${OUT:-bench_out}" && cd "${OUT:-bench_out}" && pwd)"
make -s -C oracle _build/libeu_oracle.so
python -m pytest tests -m gpu -q 2>&1 | tail -4 | tee "$OUT/pytest_gpu.log"
python __graft_entry__.py smoke 2>&1 | tail -1
python bench.py --steps 20 --warmup 3 --full 2>&1 | tail -1 > "$OUT/bench_headline.json"
cat "$OUT/bench_headline.json"
export TMPDIR=/tmp
rm -rf "$OUT/prof_headline"
(cd /tmp && rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof_headline" -- python3 "$R/bench.py" --steps 10 --warmup 2 --no-cpu-baseline > "$OUT/prof_headline.log" 2>&1)
head -4 "$OUT"/prof_headline/*/*kernel_stats.csv | cut -c1-160
