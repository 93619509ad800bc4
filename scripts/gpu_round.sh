#!/bin/bash
# One GPU-box pass: GPU tests, the default bench line, rocprofv3 kernel stats of the
# headline bench.  Each step under its own time limit, chained so a failure stops it.
set -e
O=${O:-bench_out}
mkdir -p "$O"
export TMPDIR=/tmp
timeout -k 10 600 python3 -u -m pytest tests -m gpu -x -v --timeout 120 --timeout-method thread > $O/gputest.log 2>&1
timeout -k 10 400 python3 -u bench.py --full > $O/bench.json 2> $O/bench.err
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_head -o run -- \
    python3 bench.py --full --no-cpu-baseline --api-bytes 0 --no-e2e --alt-methods "" > $O/prof_head.json 2> $O/prof_head.err
