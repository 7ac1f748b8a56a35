#!/bin/bash
# full GPU suite + smoke + the default bench line (both legs, cpu baseline)
mkdir -p results
export TMPDIR=/tmp
python -c "import __graft_entry__ as g; g.build()" > results/build.log 2>&1; tail -1 results/build.log
timeout 2400 python -m pytest tests -m gpu -q --tb=short -p no:cacheprovider --durations=8 > results/pytest_gpu.log 2>&1; echo "pytest rc=$?" >> results/pytest_gpu.log; tail -25 results/pytest_gpu.log
timeout 300 python __graft_entry__.py smoke > results/smoke.log 2>&1; echo "smoke rc=$?" >> results/smoke.log; tail -2 results/smoke.log
timeout 900 python bench.py --full > results/bench_default.json 2> results/bench_default.err; echo "bench rc=$?" >> results/bench_default.err; python - <<'PY'
import json
d=json.load(open('results/bench_default.json'))
print(d['value'], d['ms_per_step'], d['roofline']['frac'], {k:(v['launches'],v['ms']) for k,v in d['roofline']['breakdown'].items()}, 'f16x2', d.get('f16x2_leg',{}).get('value'), 'cpu', d['cpu_baseline'].get('value'), d['cpu_baseline'].get('speedup'))
PY
tail -2 results/bench_default.err
