#!/bin/bash
# config 2 alternating library variants on one box, no tests (A/B timing only)
#   usage: bash tools/gpu_r6o.sh TAG ROUNDS v1 v2 ...
OUT=${OUT:-$PWD/bench_out}
TAG=$1; R=$2; shift 2
export TMPDIR=/tmp
mkdir -p $OUT
VD=multimodal-ssl-avmnist_amd/avdino/variants
for r in $(seq $R); do
  for v in "$@"; do
    if [ $v = default ]; then unset AVDINO_LIB; else export AVDINO_LIB=$VD/libavdino_$v.so; fi
    line=$(timeout -k 10 300 python bench.py --full --no-cpu-baseline --steps 40 2>$OUT/abo_$TAG.err) || { tail -5 $OUT/abo_$TAG.err; exit 1; }
    echo "$v $(echo "$line" | python -c "import json,sys; d=json.loads(sys.stdin.readline()); r=d['roofline']; print(d['value'], d['ms_per_step'], r['kernel'][:44], r['avg_launch_us'], r.get('isolated_avg_launch_us'), r['frac'])")" | tee -a $OUT/abo_$TAG.txt
  done
done
