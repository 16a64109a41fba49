#!/bin/bash
# rocprofv3 kernel statistics of the headline bench run (with its roofline events: --full).
# Usage: bash tools/prof_kernel_stats.sh [TAG] [OUT]; writes OUT/<TAG>_kernel_stats_1gpu.csv and OUT/<TAG>_bench_under_rocprof.json
# (OUT defaults to prof_out/ in the repository root).
TAG=${1:-r03}
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${2:-$R/prof_out}
mkdir -p $OUT/prof_${TAG} && OUT=$(cd $OUT && pwd)
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_${TAG} -o ${TAG} -- python3 $R/bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --no-vae > $OUT/${TAG}_bench_under_rocprof.json 2> $OUT/${TAG}_bench_under_rocprof.err
ls $OUT/prof_${TAG}/* | head
f=$(ls $OUT/prof_${TAG}/*kernel_stats.csv $OUT/prof_${TAG}/*/*kernel_stats.csv 2>/dev/null | head -1)
cp $f $OUT/${TAG}_kernel_stats_1gpu.csv
find $OUT/prof_${TAG} -name "*kernel_trace.csv" -delete
head -12 $OUT/${TAG}_kernel_stats_1gpu.csv | cut -c1-150
tail -c 600 $OUT/${TAG}_bench_under_rocprof.json
