#!/bin/bash
# step time of the headline bench per pipeline setting (AMBC_NSEG / AMBC_CGRID), interleaved
set -e
O=${O:-bench_out}
mkdir -p "$O"
export TMPDIR=/tmp
for r in 1 2; do
for cfg in "4 1024 AMBC_ONE_ENC_STREAM=1" "4 1024 X=1" "8 1024 X=1" "6 1024 X=1" "5 1024 X=1"; do
  set -- $cfg
  env AMBC_NSEG=$1 AMBC_CGRID=$2 $3 timeout -k 10 200 python3 bench.py --full --no-cpu-baseline --api-bytes 0 --no-e2e --alt-methods "" --no-verify --steps 5 --warmup 2 > $O/seg.json 2>/dev/null
  echo "nseg=$1 cgrid=$2 $3 $(python3 -c "import json; d=json.load(open('$O/seg.json')); print(d['ms_per_step'], d['value'])")" >> $O/seg.log
done
done
