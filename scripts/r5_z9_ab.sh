#!/bin/bash
# zlib-9 A/B: base = committed, new = the change under test.  GPU suite on new first.
set -e
export TMPDIR=/tmp
O=gpurun_out/${AB_OUT:-r5z9}
mkdir -p $O
L=$PWD/adaptive-compression_amd/ambc
timeout -k 10 600 python3 -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread > $O/tests_new.log 2>&1
echo tests new ok
for rep in 1 2; do
  for lib in base new; do
    f=$L/libambc_hip.so; [ $lib = base ] && f=$L/libambc_hip_base.so
    AMBC_LIB=$f timeout -k 10 300 python3 -u scripts/kbench.py --flags 2 --msets "5;1,3,4,5" --inputs zero,random,ascii,mixed --size 268435456 --reps 2 > $O/kbench_${lib}_$rep.log 2>&1
    AMBC_LIB=$f timeout -k 10 300 python3 bench.py --full --no-cpu-baseline --api-bytes 0 --no-e2e --alt-methods "1,3,4,5z" --walk-bytes 0 --ref-walk-bytes 0 --ref-full-walk-bytes 0 --steps 3 --warmup 1 > $O/bench_${lib}_$rep.json 2> $O/bench_${lib}_$rep.err
  done
done
echo ab ok
