#!/bin/bash
# DCCRN (C3) with 1 vs 2 batches in flight, then the default bench line.
set -o pipefail
O=${OUT_DIR:-bench_out}
mkdir -p $O
for k in 1 2; do
  timeout -k 10 300 python bench.py --full --pipeline crn --steps 10 --warmup 2 --no-cpu --no-rtf --crn-inflight $k > $O/inflc_$k.json 2> $O/inflc_$k.err || exit 1
  python - "$k" "$O/inflc_$k.json" <<'PY'
import json, sys
d = json.loads(open(sys.argv[2]).read().strip().splitlines()[-1])
print('crn inflight', sys.argv[1], d['ms_per_step'], d['stage_ms_per_step'], d['value'])
PY
done
timeout -k 10 400 python bench.py --full > $O/bench_default.json 2> $O/bench_default.err || exit 1
tail -c 3000 $O/bench_default.json
