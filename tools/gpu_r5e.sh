#!/bin/bash
# Selected tests (-k filter) + bench line + graph-replay kernel trace + phase marks.
# usage: K="expr" bash tools/gpu_r5e.sh TAG "tests..."   (K optional: a pytest -k expression)
OUT=${OUT:-$PWD/bench_out}
TAG=$1; TESTS=$2
export TMPDIR=/tmp
mkdir -p $OUT
if [ -n "$TESTS" ]; then
  timeout -k 10 900 python -u -m pytest $TESTS -x -q -m gpu ${K:+-k "$K"} --timeout 300 --timeout-method thread -rf -s > $OUT/t_$TAG.log 2>&1
  rc=$?; grep -aE "^E  |passed|failed|FAILED|Error|curve|ours bf16" $OUT/t_$TAG.log | cut -c1-300 | tail -20; [ $rc -eq 0 ] || exit $rc
fi
timeout -k 10 300 python bench.py --full --no-cpu-baseline > $OUT/bench_$TAG.json 2> $OUT/bench_$TAG.err || { tail -5 $OUT/bench_$TAG.err; exit 1; }
cut -c1-330 $OUT/bench_$TAG.json
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_$TAG -o run -- \
    python bench.py --full --no-cpu-baseline --steps 20 > $OUT/bprof_$TAG.json 2> $OUT/bprof_$TAG.err || exit $?
python tools/kstats.py $OUT/prof_$TAG/run_kernel_stats.csv 40 > $OUT/ks_$TAG.txt
python tools/trace_by_grid.py $OUT/prof_$TAG/run_kernel_trace.csv 25 300 > $OUT/grid_$TAG.txt
grep -E "gemm_pair|gemm_mfma_kernel<2, 128, 256|sum_rows|all kernels" $OUT/grid_$TAG.txt | head -12
timeout -k 10 300 python tools/phase_marks.py --steps 8 > $OUT/marks_$TAG.txt 2>&1
echo "marks rc=$?"; grep -E "bwd.main_heads|heads_joined|end$|# " $OUT/marks_$TAG.txt | head
