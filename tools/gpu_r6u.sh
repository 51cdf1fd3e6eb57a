#!/bin/bash
# isolated + in-graph time of the audio conv1 apply pass: current library vs variants/libavdino_c1old.so
OUT=${OUT:-$PWD/bench_out}
export TMPDIR=/tmp
mkdir -p $OUT
K="c1_apply_codes[7168x112x112x1->8 k5]"
for r in 1 2 3; do
  for v in default c1old; do
    if [ $v = default ]; then unset AVDINO_LIB; else export AVDINO_LIB=multimodal-ssl-avmnist_amd/avdino/variants/libavdino_$v.so; fi
    line=$(timeout -k 10 300 python bench.py --full --no-cpu-baseline --steps 30 --dominant "$K" 2>$OUT/abu.err) || { tail -5 $OUT/abu.err; exit 1; }
    echo "$v $(echo "$line" | python -c "import json,sys; d=json.loads(sys.stdin.readline()); r=d['roofline']; print(d['value'], d['ms_per_step'], r['kernel'][:40], r['avg_launch_us'], r.get('isolated_avg_launch_us'))")" | tee -a $OUT/abu.txt
  done
done
