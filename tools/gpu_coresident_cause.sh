#!/bin/bash
# Re-run the measurements of profiles/r06_coresident_cause.txt on a MI355X (one GPU session, ~2 min):  bash tools/gpu_coresident_cause.sh
#   -> results/coresident_cause.txt
# Builds the three programs on the box (hipcc, ~1 min) unless tools/bin/ already holds them.
mkdir -p results tools/bin; export TMPDIR=/tmp
for t in repro_pk_fma_beside_mfma repro_coresident_bisect repro_coresident; do
  [ -x tools/bin/$t ] || hipcc --offload-arch=gfx950 -O3 -std=c++17 -I include tools/$t.cpp -o tools/bin/$t -lpthread -ldl 2> results/build_$t.err || { echo "build of $t failed"; exit 2; }
done
L=$PWD/mcvd_pytorch_amd/libmcvd_hip.so
{
echo "#### 5. the stand-alone reproducer (exit code 1 = the erratum is there)"
timeout 100 tools/bin/repro_pk_fma_beside_mfma 2; echo "exit code $?"
echo "#### 2. the instruction sequence and its variants beside the attention kernel"
VARS="0 1 2 3 4 5 6 7" timeout 200 tools/bin/repro_coresident_bisect 1.5 | grep -v "first bad"
echo "#### 3. synthetic aggressors (victim 6)"
AITER=400 AGRID=512 AGGRS="1 2 3 4 5 6 7 8 9 10 11 12 13" VARS="6" timeout 300 tools/bin/repro_coresident_bisect 2 | grep -v "first bad"
echo "#### 4. the matrix instruction inside the victim's own wave; other dual-read forms"
AITER=400 AGRID=512 AGGRS="0 11" VARS="8 12 13 14 15 16 17" timeout 300 tools/bin/repro_coresident_bisect 1.5 | grep -v "first bad"
echo "#### 6. the library's former victims through the C ABI, and two streams of one process through the Python stack"
for sh in 0 2 3; do ONLY_LIB=1 VICTIM_SHAPE=$sh timeout 100 tools/bin/repro_coresident 2 $L | grep -v "^# aggressor attn\|first bad"; done
SECS=2 timeout 300 python tools/diag_concurrent_streams.py 2>&1 | grep -v "^   diff\|amdgpu.ids"
} > results/coresident_cause.txt 2>&1
tail -3 results/coresident_cause.txt
