#!/bin/bash
# same-box A/B of several zlib-9 variants: base (libambc_hip.so) against each
# adaptive-compression_amd/ambc/libambc_hip_x<k>.so given in XS (e.g. XS="g4 g16");
# {1,3,4,5z} leg and like_reference() walk, then the zlib-9 GPU tests per variant
set -e
O=gpurun_out/${EV_OUT:-r6z9abn}
mkdir -p $O
L=$PWD/adaptive-compression_amd/ambc
B="python3 bench.py --full --no-cpu-baseline --api-bytes 0 --no-e2e --walk-bytes 0 --ref-full-walk-bytes 0 --ref-walk-check-bytes 0 --steps 2 --warmup 1 --alt-methods 1,3,4,5z --no-verify"
for r in 1 2; do
  timeout -k 10 300 $B > $O/base_$r.json 2> $O/base_$r.err
  for x in $XS; do
    AMBC_LIB=$L/libambc_hip_x$x.so timeout -k 10 300 $B > $O/${x}_$r.json 2> $O/${x}_$r.err
  done
done
for x in $XS; do
  AMBC_LIB=$L/libambc_hip_x$x.so timeout -k 10 600 python3 -u -m pytest -x -q --timeout 300 --timeout-method thread tests/test_gpu_zlib9.py > $O/tests_$x.log 2>&1
done
echo ok
