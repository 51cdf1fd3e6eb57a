#!/bin/bash
# Selected GPU tests + bench line + config-5 probe line + graph-replay kernel trace.
# usage: bash tools/gpu_r5b.sh TAG "tests/test_a.py tests/test_b.py"
OUT=${OUT:-$PWD/bench_out}
TAG=$1
TESTS=$2
export TMPDIR=/tmp
mkdir -p $OUT
if [ -n "$TESTS" ]; then
  timeout -k 10 900 python -u -m pytest $TESTS -x -q -m gpu --timeout 300 --timeout-method thread -rf > $OUT/t_$TAG.log 2>&1
  rc=$?; grep -aE "^E  |passed|failed|FAILED|Error" $OUT/t_$TAG.log | cut -c1-300 | tail -20; [ $rc -eq 0 ] || exit $rc
fi
timeout -k 10 300 python bench.py --full --no-cpu-baseline > $OUT/bench_$TAG.json 2> $OUT/bench_$TAG.err || { tail -5 $OUT/bench_$TAG.err; exit 1; }
cut -c1-330 $OUT/bench_$TAG.json
if [ -n "$PROBE" ]; then
  timeout -k 10 300 python bench.py --full --no-cpu-baseline --mode semi_supervised --probe --steps 10 --warmup 3 > $OUT/bench_probe_$TAG.json 2> $OUT/bench_probe_$TAG.err || { tail -5 $OUT/bench_probe_$TAG.err; exit 1; }
  python -c "import json; d=json.loads(open('$OUT/bench_probe_$TAG.json').readline()); print(d['value'], d['ms_per_step'], d['probe'])"
fi
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_$TAG -o run -- \
    python bench.py --full --no-cpu-baseline --steps 20 > $OUT/bprof_$TAG.json 2> $OUT/bprof_$TAG.err || exit $?
python tools/kstats.py $OUT/prof_$TAG/run_kernel_stats.csv 40 > $OUT/ks_$TAG.txt
python tools/trace_by_grid.py $OUT/prof_$TAG/run_kernel_trace.csv 25 60 > $OUT/grid_$TAG.txt
head -12 $OUT/ks_$TAG.txt | cut -c1-150; grep -E "sum_rows|all kernels" $OUT/grid_$TAG.txt
