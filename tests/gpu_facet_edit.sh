#!/bin/bash
# The device form of the PTO mask / lens crop edit on a GPU box: its tests, the two load routes timed against
# each other, and a kernel trace of one edited load. Every step that uses the GPU runs under a time limit of
# its own and the next one starts only if it ended well.
R="$(cd "$(dirname "$0")/.." && pwd)"; cd "$R"
OUT="$(mkdir -p "${OUT:-bench_out}" && cd "${OUT:-bench_out}" && pwd)"
export TMPDIR=/tmp
set -o pipefail
make -s -C oracle _build/libeu_oracle.so &&
timeout -k 10 500 python -m pytest tests/test_gpu_facet_edit.py tests/test_facet_alpha_rows.py -m "gpu or not gpu" -q 2>&1 | tee "$OUT/pytest_facet_edit.log" | tail -15 &&
timeout -k 10 300 python tools/facet_edit_time.py --out "$OUT/facet_edit_load_times.json" &&
rm -rf "$OUT/prof_facet_edit" &&
(cd /tmp && timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof_facet_edit" -- python3 "$R/tools/facet_edit_time.py" --only b > "$OUT/prof_facet_edit.log" 2>&1) &&
head -8 "$OUT"/prof_facet_edit/*/*kernel_stats.csv | cut -c1-200
