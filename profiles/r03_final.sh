#!/bin/bash
# Round 3, final tree: the bench lines and rocprofv3 summaries committed as profiles/<tag>_* (run on the GPU box from the repo root):
#   bash profiles/r03_final.sh <tag> profile   -> the rocprofv3 passes (summarised afterwards by profiles/summarize.py / pmc_summary.py)
#   bash profiles/r03_final.sh <tag> bench     -> the bench lines (their roofline counters come from the committed summaries)
set -x
T=${1:-r03zz}
if [ "$2" = profile ]; then
  timeout -k 10 500 bash profiles/collect.sh $T || exit 1
  timeout -k 10 300 bash profiles/collect_pmc.sh $T
  exit $?
fi
OUT=${OUT:-bench_out}                # where the bench lines go
mkdir -p $OUT
timeout -k 10 300 python bench.py --full --gpus 1 --steps 20 --warmup 5 > $OUT/${T}_bench.json 2> $OUT/${T}_bench.err || exit 1
timeout -k 10 300 python bench.py --full --assoc mcf --steps 10 --warmup 2 > $OUT/${T}_bench_mcf.json 2>> $OUT/${T}_bench.err || exit 1
timeout -k 10 300 python bench.py --full --input host --steps 20 --warmup 5 --cpu-frames 0 > $OUT/${T}_bench_host.json 2>> $OUT/${T}_bench.err || exit 1
for w in assoc-c3 assoc-c4; do for a in mcf hungarian; do
  timeout -k 10 300 python bench.py --full --workload $w --assoc $a --steps 5 --warmup 2 > $OUT/${T}_bench_${w}_${a}.json 2>> $OUT/${T}_bench.err || exit 1
done; done
timeout -k 10 300 python bench.py --full --gpus 2 --backend gloo --single-device --assoc mcf --frames 132 --steps 3 --warmup 1 --no-verify > $OUT/${T}_bench_2ranks_mcf.json 2>> $OUT/${T}_bench.err || exit 1
