#!/bin/bash
# Selected GPU tests (verbose, one pytest process), then the default bench line.
#   usage: bash tools/gpu_sel.sh TAG [pytest args...]
OUT=${OUT:-$PWD/bench_out}
TAG=$1; shift
export TMPDIR=/tmp
mkdir -p $OUT
timeout -k 10 900 python -u -m pytest "$@" -v -s -m gpu --timeout 300 --timeout-method thread -rf \
    > $OUT/sel_$TAG.log 2>&1
rc=$?; echo "tests rc=$rc"; grep -aE "PASSED|FAILED|ERROR|^E  |passed|failed" $OUT/sel_$TAG.log | cut -c1-250 | tail -40
[ $rc -le 1 ] || exit $rc
timeout -k 10 300 python bench.py --full --no-cpu-baseline > $OUT/bench_$TAG.json 2> $OUT/bench_$TAG.err
echo "bench rc=$?"; cut -c1-400 $OUT/bench_$TAG.json
