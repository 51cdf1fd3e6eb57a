#!/bin/bash
# The default bench line (in-graph span timing of the watched launches) and rocprofv3 kernel
# stats of the same command, for the agreement check of roofline.avg_launch_us.
#   usage: bash tools/gpu_span.sh TAG [bench args...]
OUT=${OUT:-$PWD/bench_out}
TAG=$1; shift
export TMPDIR=/tmp
mkdir -p $OUT
timeout -k 10 300 python bench.py --full --no-cpu-baseline "$@" > $OUT/bench_$TAG.json 2> $OUT/bench_$TAG.err || { tail -20 $OUT/bench_$TAG.err; exit 1; }
OUT=$OUT python - "$TAG" <<'PY'
import json, os, sys
d = json.load(open(os.path.join(os.environ["OUT"], f"bench_{sys.argv[1]}.json")))
print(d["value"], d["ms_per_step"])
for k in ("roofline", "roofline_hbm"):
    r = d.get(k) or {}
    print(k, r.get("kernel"), "avg", r.get("avg_launch_us"), "eager", r.get("eager_avg_launch_us"),
          "iso", r.get("isolated_avg_launch_us"), "frac", r.get("frac"), r.get("timing"))
PY
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_$TAG -o run -- \
    python bench.py --full --no-cpu-baseline "$@" > $OUT/bprof_$TAG.json 2> $OUT/bprof_$TAG.err || exit $?
python tools/kstats.py $OUT/prof_$TAG/run_kernel_stats.csv 12 > $OUT/ks_$TAG.txt
cut -c1-160 $OUT/ks_$TAG.txt
