#!/bin/bash
# The whole -m gpu suite in one pytest process, then the default bench line.
#   usage: bash tools/gpu_suite.sh TAG
OUT=${OUT:-$PWD/bench_out}
TAG=$1
export TMPDIR=/tmp
mkdir -p $OUT
timeout -k 10 1000 python -u -m pytest tests -q -m gpu --timeout 300 --timeout-method thread -rf -s \
    > $OUT/suite_$TAG.log 2>&1
rc=$?; echo "suite rc=$rc"; grep -aE "^E  |passed|failed|FAILED" $OUT/suite_$TAG.log | cut -c1-300 | tail -30
[ $rc -le 1 ] || exit $rc
timeout -k 10 300 python bench.py --full --no-cpu-baseline > $OUT/bench_$TAG.json 2> $OUT/bench_$TAG.err
echo "bench rc=$?"; cut -c1-300 $OUT/bench_$TAG.json
