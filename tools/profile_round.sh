#!/bin/bash
# Round profile of the bench command: kernel trace + stats (csv), then the HBM-traffic counters in their own passes.
# usage (on the GPU box): tools/profile_round.sh r01   -> $OUT/prof_<tag>/... ($OUT defaults to out/), summaries printed by the tools afterwards
TAG=${1:-rXX}
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$R/out}; mkdir -p "$OUT"; export OUT
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_$TAG -o k -- python $R/bench.py --full --steps 5 --warmup 2 > $OUT/prof_${TAG}_bench.log 2>&1
for C in FETCH_SIZE WRITE_SIZE; do
  rocprofv3 --kernel-trace --pmc $C --output-format csv -d $OUT/pmc_$TAG/$C -o p -- python $R/bench.py --steps 2 --warmup 1 --no-cpu-baseline --no-roofline > $OUT/pmc_${TAG}_$C.log 2>&1
done
ls $OUT/prof_$TAG $OUT/pmc_$TAG/*
