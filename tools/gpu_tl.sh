#!/bin/bash
# bench line + one-step per-stream timeline and kernel stats of the default config-2 step.
#   usage: bash tools/gpu_tl.sh TAG [env assignments...]
OUT=${OUT:-$PWD/bench_out}
TAG=$1; shift
export TMPDIR=/tmp
mkdir -p $OUT
env "$@" timeout -k 10 300 python bench.py --full --no-cpu-baseline --steps 30 > $OUT/bench_$TAG.json 2> $OUT/bench_$TAG.err || exit $?
cut -c1-200 $OUT/bench_$TAG.json
env "$@" timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_$TAG -o run -- \
    python bench.py --full --steps 10 --warmup 3 --no-cpu-baseline > $OUT/b_$TAG.log 2>&1 || exit $?
python tools/timeline.py $OUT/prof_$TAG/run_kernel_trace.csv > $OUT/tl_$TAG.txt
python tools/kstats.py $OUT/prof_$TAG/run_kernel_stats.csv 40 > $OUT/ks_$TAG.txt
head -4 $OUT/tl_$TAG.txt
