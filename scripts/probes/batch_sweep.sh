#!/bin/bash
# bench over the batch size, with per-kernel times (--full); stops at the first failing run
T=${TMPDIR:-/tmp}
for B in 16 32 48 50 56 64 80 96 128; do
  timeout -k 10 200 python3 bench.py --batch $B --steps 10 --full --no-cpu-baseline --no-variants > $T/bs_$B.json 2>$T/bs.err || { tail -3 $T/bs.err; exit 1; }
  python3 -c "
import json; d=json.load(open('$T/bs_$B.json')); print('B=$B', round(d['value']), 'traj/s', round(d['ms_per_step'],3), 'ms', {k: round(v['avg_ms']*1e3,1) for k,v in d['roofline']['kernels'].items()})"
done
