#!/bin/bash
mkdir -p results
export TMPDIR=/tmp
python -c "import __graft_entry__ as g; g.build()" > results/build.log 2>&1; tail -1 results/build.log
timeout 2400 python -m pytest tests -m gpu -q --tb=short -p no:cacheprovider --durations=15 > results/pytest_gpu.log 2>&1; echo "pytest rc=$?" >> results/pytest_gpu.log; tail -45 results/pytest_gpu.log
timeout 300 python __graft_entry__.py smoke > results/smoke.log 2>&1; echo "smoke rc=$?" >> results/smoke.log; tail -2 results/smoke.log
timeout 300 python tests/gpu_diag.py hostloop > results/hostloop.log 2>&1; cat results/diag_hostloop.txt; tail -2 results/hostloop.log
