#!/bin/bash
# The whole -m gpu suite in one pytest process, then the default bench line.  usage: bash tools/gpu_suite5.sh TAG
OUT=${OUT:-$PWD/bench_out}
TAG=$1
export TMPDIR=/tmp
mkdir -p $OUT
timeout -k 10 1100 python -u -m pytest tests -q -m gpu --timeout 300 --timeout-method thread -rf > $OUT/suite_$TAG.log 2>&1
rc=$?; grep -aE "^E  |passed|failed|FAILED|Error" $OUT/suite_$TAG.log | cut -c1-300 | tail -25; [ $rc -eq 0 ] || exit $rc
timeout -k 10 300 python bench.py --full --no-cpu-baseline > $OUT/bench_$TAG.json 2> $OUT/bench_$TAG.err || { tail -5 $OUT/bench_$TAG.err; exit 1; }
cut -c1-330 $OUT/bench_$TAG.json
