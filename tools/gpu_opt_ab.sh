#!/bin/bash
# same-box A/B of one context option through bench.py: bash tools/gpu_opt_ab.sh <option> [configs...]   -> results/ab_<option>.txt
export TMPDIR=/tmp; mkdir -p results
OPT=$1; shift
: > results/ab_$OPT.txt
for c in ${@:-smmnist_big5_ngf96}; do
for rep in 1 2; do for v in 0 1; do
  MCVD_BENCH_OPTS=$OPT=$v timeout 600 python bench.py --full --config $c --steps 2 --warmup 1 --no-cpu-baseline --no-f16x2-leg > results/bench_ab.json 2> results/bench_ab.err
  python - <<PY | tee -a results/ab_$OPT.txt
import json
d=json.load(open('results/bench_ab.json'))
print('$c $OPT=$v', d['value'], 'frames/s', d['ms_per_step'], 'ms/step', d['valid'])
PY
done; done; done
