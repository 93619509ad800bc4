#!/bin/bash
# rocprofv3 kernel stats of the headline bench (no alt leg) and of the DEFLATE
# method-set leg, each in its own run so every kernel's average is one workload.
set -e
O=${O:-bench_out}
mkdir -p "$O"
export TMPDIR=/tmp
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_head -o run -- \
    python3 bench.py --full --no-cpu-baseline --api-bytes 0 --no-e2e --alt-methods "" > $O/prof_head.json 2> $O/prof_head.err
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_defl -o run -- \
    python3 bench.py --full --no-cpu-baseline --api-bytes 0 --no-e2e --alt-methods "" --methods 1,3,4,5 > $O/prof_defl.json 2> $O/prof_defl.err
