#!/bin/bash
# Round-end evidence: full -m gpu suite, smoke(), default bench line (CPU baseline included),
# rocprof kernel stats of the graph-replayed bench and of the same bench eager (whose average
# per launch is what bench.py's roofline events time: eager steps after the timed region).
OUT=${OUT:-$PWD/bench_out}
TAG=$1
export TMPDIR=/tmp
mkdir -p $OUT
timeout -k 10 1500 python -u -m pytest tests -q -m gpu --timeout 300 --timeout-method thread -rf > $OUT/final_tests_$TAG.log 2>&1
rc=$?; grep -aE "^E  |passed|failed|FAILED" $OUT/final_tests_$TAG.log | cut -c1-300 | tail -20; [ $rc -eq 0 ] || exit $rc
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > $OUT/smoke_$TAG.log 2>&1 || { tail -20 $OUT/smoke_$TAG.log; exit 1; }
tail -1 $OUT/smoke_$TAG.log
timeout -k 10 600 python bench.py --full > $OUT/bench_final_$TAG.json 2> $OUT/bench_final_$TAG.err || { tail -5 $OUT/bench_final_$TAG.err; exit 1; }
cut -c1-300 $OUT/bench_final_$TAG.json
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_final_$TAG -o run -- \
    python bench.py --full --no-cpu-baseline > $OUT/bprof_final_$TAG.json 2> $OUT/bprof_final_$TAG.err || exit $?
python tools/kstats.py $OUT/prof_final_$TAG/run_kernel_stats.csv 40 > $OUT/ks_final_$TAG.txt
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_eager_$TAG -o run -- \
    python bench.py --full --steps 10 --warmup 3 --no-graph --no-cpu-baseline > $OUT/bprof_eager_$TAG.json 2> $OUT/bprof_eager_$TAG.err || exit $?
python tools/kstats.py $OUT/prof_eager_$TAG/run_kernel_stats.csv 40 > $OUT/ks_eager_$TAG.txt
head -4 $OUT/ks_final_$TAG.txt | cut -c1-150; head -4 $OUT/ks_eager_$TAG.txt | cut -c1-150
