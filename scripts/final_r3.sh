#!/bin/bash
# end-of-session check: smoke(), the GPU suite, the default bench line
set -e
O=${O:-bench_out}
mkdir -p "$O"
export TMPDIR=/tmp
mkdir -p $O/final
timeout -k 10 300 python3 -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > $O/final/smoke.log 2>&1
timeout -k 10 600 python3 -u -m pytest tests -m gpu -x -v --timeout 200 --timeout-method thread > $O/final/gputest.log 2>&1
timeout -k 10 500 python3 -u bench.py --full > $O/final/bench.json 2> $O/final/bench.err
