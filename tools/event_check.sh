#!/bin/bash
# HIP-event kernel times (bench.py sequential pass) next to a rocprofv3 trace of the same command.
set -o pipefail
export TMPDIR=/tmp
R=$(pwd)
O=${OUT_DIR:-$R/bench_out}
mkdir -p $O
timeout -k 10 200 python bench.py --full --steps 20 --warmup 3 --no-cpu --no-c3 --no-rtf > $O/ev_bench.json 2> $O/ev_bench.err || exit 1
python -c "import json; d=json.loads(open('$O/ev_bench.json').read().strip().splitlines()[-1]); print(d['ms_per_step'], d['kernel_ms_per_step'])"
cd /tmp && timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/ev_trace -o run -- python3 $R/bench.py --full --steps 20 --warmup 3 --no-cpu --no-c3 --no-rtf > $O/ev_trace.log 2>&1 || exit 1
cd $R && head -4 $O/ev_trace/run_kernel_stats.csv | cut -c1-160
grep -h '^{' $O/ev_trace.log | python -c "import json,sys; d=json.loads(sys.stdin.read().strip().splitlines()[-1]); print('under tracer', d['ms_per_step'], d['kernel_ms_per_step'])"
