#!/bin/bash
# Batches in flight (bench.py --inflight): 1 (sequential) vs 2 vs 3.
set -o pipefail
O=${OUT_DIR:-bench_out}
mkdir -p $O
for k in ${INFL:-1 2 3 2}; do
  timeout -k 10 200 python bench.py --full --steps 20 --warmup 3 --no-cpu --no-c3 --no-rtf --inflight $k > $O/infl_$k.json 2> $O/infl_$k.err || exit 1
  python - "$k" "$O/infl_$k.json" <<'PY'
import json, sys
d = json.loads(open(sys.argv[2]).read().strip().splitlines()[-1])
print('inflight', sys.argv[1], d['ms_per_step'], d['kernel_ms_per_step'], d['value'])
PY
done
