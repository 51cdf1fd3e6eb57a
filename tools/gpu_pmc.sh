#!/bin/bash
# HBM traffic of the bench's dominant launch: two counter passes (FETCH_SIZE and WRITE_SIZE do
# not fit one TCC pass), each replaying only that launch K times.  usage: bash tools/gpu_pmc.sh TAG
OUT=${OUT:-$PWD/bench_out}
TAG=$1
export TMPDIR=/tmp
mkdir -p $OUT
K=20
# the roofline kernel of the bench line (bench.py --full, written to $OUT/bench_$TAG.json by
# gpu_suite.sh / gpu_sel.sh / gpu_prof.sh), so the counters
# measure exactly the launch the bench reports
# (or pass it as DOM=... when the bench ran elsewhere)
DOM=${DOM:-$(python -c "import json,sys; print(json.loads(open('$OUT/bench_$TAG.json').readline())['roofline']['kernel'])")}
echo "dominant: $DOM"
timeout -k 10 600 rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $OUT/pmcF_$TAG -o run -- \
    python bench.py --steps 1 --warmup 2 --no-cpu-baseline --probe-dominant $K --dominant "$DOM" > $OUT/probeF_$TAG.json 2> $OUT/probeF_$TAG.err \
&& timeout -k 10 600 rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d $OUT/pmcW_$TAG -o run -- \
    python bench.py --steps 1 --warmup 2 --no-cpu-baseline --probe-dominant $K --dominant "$DOM" > $OUT/probeW_$TAG.json 2> $OUT/probeW_$TAG.err \
&& python tools/pmc_traffic.py $OUT/probeF_$TAG.json $OUT/pmcF_$TAG $OUT/pmcW_$TAG $OUT/traffic_$TAG.json
echo "pmc rc=$?"
