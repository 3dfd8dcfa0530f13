#!/bin/bash
# Kernel-variant experiments on the GPU box (through gpurun):  bash scripts/variants.sh OUTFILE "ENV1=a ENV2=b" "ENV1=c" ...
# Each variant is one bench.py process (the knobs are read once per process); prints ms_per_step and the per-kernel
# HIP-event times of bench.py's roofline leg.
OUT=$1; shift
RESULTS=${RESULTS:-results}   # where the records go (a directory under the repository root, git-ignored)
mkdir -p $RESULTS
: > $RESULTS/$OUT
for v in "$@"; do
  echo "== $v" >> $RESULTS/$OUT
  env $v python bench.py --full --no-cpu-baseline --steps 8 --warmup 2 --distinct 16 ${BENCH_ARGS} 2>> $RESULTS/$OUT.err | python -c "
import json,sys
d=json.loads(sys.stdin.read().strip().splitlines()[-1])
print('value', d['value'], 'ms_per_step', d['ms_per_step'], 'variant', (d.get('variant') or {}).get('ms_per_step'))
k=d['roofline']['kernels_ms_per_step']
print(' '.join('%s=%.3f'%(a,b) for a,b in list(k.items())[:14]))
" >> $RESULTS/$OUT
done
cat $RESULTS/$OUT
