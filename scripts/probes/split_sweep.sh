#!/bin/bash
# k_linearize: shared-walk 4-wavefront form (with the fused finish) against the replicated 2-wavefront form (+ k_finish_step)
# over the batch size; per-kernel times need --full; stops at the first failing run
T=${TMPDIR:-/tmp}
for B in ${BATCHES:-32 64 128 256 512}; do for S in 2 4; do
  GPMP2MI_LIN_SPLIT=$S timeout -k 10 200 python3 bench.py --batch $B --steps 10 --full --no-cpu-baseline --no-variants > $T/ss.json 2>$T/ss.err || { tail -3 $T/ss.err; exit 1; }
  python3 -c "
import json; d=json.load(open('$T/ss.json')); print('B=$B split=$S', round(d['value']), 'traj/s', {k: round(v['avg_ms']*1e3,1) for k,v in d['roofline']['kernels'].items()})"
done; done
