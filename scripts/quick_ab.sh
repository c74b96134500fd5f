#!/bin/bash
# quick A/B on the GPU box: parity tests of the plan path, then the two bench regimes with per-kernel times
set -o pipefail
# logs and bench lines go to $OUT_DIR (default: $TMPDIR/quick_ab); per-kernel times need bench.py --full
O=${OUT_DIR:-${TMPDIR:-/tmp}/quick_ab}
mkdir -p $O
T=${1:-"tests/test_gpu_plan.py tests/test_gpu_robots.py tests/test_gpu_planner_api.py"}
timeout -k 10 600 python3 -m pytest $T -m gpu -x -q > $O/ab_tests.log 2>&1; rc=$?; echo "pytest rc=$rc"; tail -4 $O/ab_tests.log
if [ $rc -eq 124 ] || [ $rc -ge 128 ]; then echo "the tests were killed or aborted: no further GPU step"; exit 1; fi
for B in 64 1024; do
  timeout -k 10 300 python3 bench.py --batch $B --steps 10 --full --no-cpu-baseline --no-variants > $O/ab_b$B.json 2> $O/ab_b$B.err || { tail -5 $O/ab_b$B.err; exit 1; }
  python3 -c "
import json; d=json.load(open('$O/ab_b$B.json')); print('B=$B', round(d['value']), 'traj/s', round(d['ms_per_step'],3), 'ms', {k: round(v['avg_ms']*1e3,1) for k,v in d['roofline']['kernels'].items()})"
done
