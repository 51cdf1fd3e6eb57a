#!/bin/bash
# Selected GPU test files, the bench line, then rocprof kernel stats of the graph-replayed bench
# (+ per-stream timeline) and of the eager bench.
#   usage: bash tools/gpu_prof.sh TAG [test files...]
OUT=${OUT:-$PWD/bench_out}
TAG=$1; shift
export TMPDIR=/tmp
mkdir -p $OUT
if [ $# -gt 0 ]; then
  timeout -k 10 600 python -u -m pytest "$@" -q -m gpu --timeout 120 --timeout-method thread -rf \
      > $OUT/sel_$TAG.log 2>&1
  rc=$?; echo "tests rc=$rc"; grep -aE "^E  |passed|failed|FAILED" $OUT/sel_$TAG.log | cut -c1-300 | tail -20
  [ $rc -le 1 ] || exit $rc
fi
timeout -k 10 300 python bench.py --full --no-cpu-baseline > $OUT/bench_$TAG.json 2> $OUT/bench_$TAG.err || exit $?
cut -c1-200 $OUT/bench_$TAG.json
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_$TAG -o run -- \
    python bench.py --full --steps 10 --warmup 3 --no-cpu-baseline > $OUT/b_$TAG.log 2>&1 || exit $?
python tools/timeline.py $OUT/prof_$TAG/run_kernel_trace.csv > $OUT/tl_$TAG.txt
python tools/kstats.py $OUT/prof_$TAG/run_kernel_stats.csv 60 > $OUT/ks_$TAG.txt
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_eager_$TAG -o run -- \
    python bench.py --full --steps 10 --warmup 3 --no-graph --no-cpu-baseline > $OUT/be_$TAG.log 2>&1 || exit $?
python tools/kstats.py $OUT/prof_eager_$TAG/run_kernel_stats.csv 60 > $OUT/kse_$TAG.txt
head -4 $OUT/tl_$TAG.txt
