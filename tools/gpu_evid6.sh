#!/bin/bash
# Round-6 evidence: smoke(), the default bench line (CPU baseline included), rocprof kernel
# stats of the graph-replayed bench.   usage: bash tools/gpu_evid6.sh TAG
ROOT=$PWD
OUT=${OUT:-$PWD/bench_out}
TAG=$1
export TMPDIR=/tmp
mkdir -p $OUT
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > $OUT/smoke_$TAG.log 2>&1 || { tail -20 $OUT/smoke_$TAG.log; exit 1; }
tail -1 $OUT/smoke_$TAG.log
timeout -k 10 400 python bench.py --full > $OUT/bench_$TAG.json 2> $OUT/bench_$TAG.err || { tail -5 $OUT/bench_$TAG.err; exit 1; }
cut -c1-600 $OUT/bench_$TAG.json; grep "in-graph candidates" $OUT/bench_$TAG.err | cut -c1-600
cd /tmp && timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_$TAG -o run -- \
    python $ROOT/bench.py --full --no-cpu-baseline --steps 30 > $OUT/bprof_$TAG.json 2> $OUT/bprof_$TAG.err || exit $?
cd $ROOT && python tools/kstats.py $OUT/prof_$TAG/run_kernel_stats.csv 40 > $OUT/ks_$TAG.txt
head -6 $OUT/ks_$TAG.txt | cut -c1-160
