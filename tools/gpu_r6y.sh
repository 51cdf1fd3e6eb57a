#!/bin/bash
# config 5 fp8: the 56^2 layer backward through the fused bf16 launch vs the MX kernels
OUT=${OUT:-$PWD/bench_out}
export TMPDIR=/tmp
mkdir -p $OUT
for r in 1 2 3; do
  for spec in "-" "ConvBranch.FP8_FUSED_BWD=True"; do
    if [ "$spec" = "-" ]; then args=(); else args=($spec); fi
    v=$(timeout -k 10 300 python tools/ab_attr.py "${args[@]}" -- --full --no-cpu-baseline --steps 20 --mode semi_supervised --dtype fp8 2>$OUT/aby.err | python -c "import json,sys; d=json.loads(sys.stdin.readline()); print(d['value'], d['ms_per_step'], d['roofline']['kernel'][:44], d['roofline']['avg_launch_us'], d['roofline']['frac'])") || { tail -5 $OUT/aby.err; exit 1; }
    echo "[$spec] $v" | tee -a $OUT/aby.txt
  done
done
