#!/bin/bash
# Bench line + PMC traffic of the launches the bench now reports (the 14^2 and 56^2 weight
# gradients, replayed alone) + whole-step PMC bytes.  usage: bash tools/gpu_r5base.sh TAG
OUT=${OUT:-$PWD/bench_out}
TAG=$1
export TMPDIR=/tmp
mkdir -p $OUT
timeout -k 10 300 python bench.py --full --no-cpu-baseline > $OUT/bench_$TAG.json 2> $OUT/bench_$TAG.err || { tail -5 $OUT/bench_$TAG.err; exit 1; }
cut -c1-400 $OUT/bench_$TAG.json
rm -f $OUT/traffic_$TAG.json
for DOM in "cl_conv_wgrad[7168x14x14x32->64 k5p2 torch.bfloat16] @side" "cl_conv_wgrad[7168x56x56x8->16 k5p2 torch.bfloat16] @side"; do
  for C in FETCH_SIZE WRITE_SIZE; do
    timeout -s KILL 180 rocprofv3 --pmc $C --kernel-trace --output-format csv -d $OUT/pmc${C:0:1}_$TAG -o run -- \
        python bench.py --steps 1 --warmup 2 --no-cpu-baseline --probe-dominant 20 --dominant "$DOM" \
        > $OUT/probe${C:0:1}_$TAG.json 2> $OUT/probe${C:0:1}_$TAG.err
    rc=$?; echo "$DOM $C rc=$rc"; [ $rc -eq 0 ] || exit $rc
  done
  python tools/pmc_traffic.py $OUT/probeF_$TAG.json $OUT/pmcF_$TAG $OUT/pmcW_$TAG $OUT/traffic_$TAG.json || exit 1
  rm -rf $OUT/pmcF_$TAG $OUT/pmcW_$TAG
done
bash tools/gpu_pmc_step.sh $TAG
