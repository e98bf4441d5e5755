#!/bin/bash
set -e
R="$(cd "$(dirname "$0")/.." && pwd)"
cd "$R"; OUT="${OUT:-bench_out}"; mkdir -p "$OUT"
make -s -C oracle _build/libeu_oracle.so
python -m pytest tests -m gpu -q -x 2>&1 | tail -5 | tee "$OUT/pytest_gpu.log"
for w in headline probe_smallsrc probe_bilinear; do
  EU_HIP_DIRECT=1 python bench.py --workload $w --steps 10 --no-cpu-baseline 2>&1 | tail -1 > "$OUT/ab_${w}_direct.json"
  python bench.py --workload $w --steps 10 --no-cpu-baseline 2>&1 | tail -1 > "$OUT/ab_${w}_lds.json"
done
python bench.py --steps 20 --full 2>&1 | tail -1 > "$OUT/bench_headline.json"
python - "$OUT" <<'PY'
import json,glob,os,sys
o=sys.argv[1]
for f in sorted(glob.glob(os.path.join(o,'ab_*.json')))+[os.path.join(o,'bench_headline.json')]:
    d=json.loads(open(f).read()); print(f, d['roofline']['kernel_ms'], d['value'], d['roofline']['frac'], d.get('cpu_baseline',{}).get('gpu_rows_bit_identical'))
PY
