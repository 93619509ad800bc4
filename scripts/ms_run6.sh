#!/bin/bash
set -e
O=${O:-bench_out}
mkdir -p "$O"
export TMPDIR=/tmp
mkdir -p $O/ms6
timeout -k 10 500 python3 -u -m pytest tests/test_gpu_parity.py -m gpu -x -q --timeout 200 --timeout-method thread -k "multisize or like_reference or host_scored" > $O/ms6/tests.log 2>&1
timeout -k 10 400 python3 bench.py --full --no-cpu-baseline --api-bytes 0 --no-e2e --alt-methods "" --steps 3 --warmup 1 > $O/ms6/bench.json 2> $O/ms6/bench.err
