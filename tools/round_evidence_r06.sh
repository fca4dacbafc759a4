#!/bin/bash
# Round-6 evidence on the GPU box, everything from ONE build: the full GPU test suite, kernel trace + stats and the counter passes of the
# bench command (tools/profile_round.sh), idle time inside the replayed step (tools/graph_gaps.py), the per-shape timing, the lines of the
# other BASELINE configurations with the DEFAULT protocol (100 timed steps after 20 warm-up; config 3 = AtomNAS-A, forced 30 % shrink,
# --allow-untrained: the cross entropy on the fixed batch rises for the first steps after the shrink), the supernet fed by the GPU input
# pipeline, smoke(), and last the default bench line (after the PMC summaries have been written to profiles/ with this build's digest).
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$R/out}; mkdir -p "$OUT"; export OUT
cd $R
T=r06
timeout 1500 python -m pytest tests -q -m gpu -p no:cacheprovider 2>&1 | tail -12 > $OUT/${T}_pytest_full.log
bash tools/profile_round.sh $T > $OUT/evidence_$T.log 2>&1
(cd /tmp && export TMPDIR=/tmp && timeout 600 rocprofv3 --kernel-trace --pmc SQ_INSTS_VALU_MFMA_MOPS_BF16 SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES --output-format csv -d $OUT/pmc_$T/MFMA -o p -- python $R/bench.py --steps 2 --warmup 1 --no-cpu-baseline --no-roofline > $OUT/pmc_${T}_MFMA.log 2>&1)
python tools/rocprof_summary.py $OUT/prof_$T/k_kernel_trace.csv > $OUT/${T}_bench_bs256_kernel_summary.txt 2>&1
cp $(find $OUT/prof_$T -name "*kernel_stats.csv" | head -1) $OUT/${T}_bench_bs256_kernel_stats.csv 2>/dev/null
(cd /tmp && export TMPDIR=/tmp && timeout 600 rocprofv3 --kernel-trace --output-format csv -d $OUT/gaps_$T -o k -- python $R/bench.py --steps 6 --warmup 3 --no-cpu-baseline --no-roofline > /dev/null 2>&1)
python tools/graph_gaps.py $(dirname $(find $OUT/gaps_$T -name "*kernel_trace.csv" | head -1)) 3 > $OUT/${T}_graph_gaps.txt 2>&1
rm -rf $OUT/gaps_$T
python tools/pmc_traffic.py $OUT/pmc_$T > profiles/${T}_pmc_traffic.json 2> $OUT/${T}_pmc_traffic.log
python tools/pmc_mfma.py $OUT/pmc_$T/MFMA > profiles/${T}_pmc_mfma.json 2> $OUT/${T}_pmc_mfma.log
cp profiles/${T}_pmc_traffic.json profiles/${T}_pmc_mfma.json $OUT/ 2>/dev/null
DETAIL=1 timeout 300 python tools/bringup.py 256 > $OUT/${T}_bs256_per_shape_timing.txt 2>&1
timeout 400 python bench.py --full --model atomnas_a_supernet --no-cpu-baseline > $OUT/${T}_bench_cfg2_atomnas_a_supernet.json 2> $OUT/${T}_bench_cfg2.err
timeout 400 python bench.py --full --model atomnas_a_supernet --shrink 0.3 --allow-untrained --no-cpu-baseline > $OUT/${T}_bench_cfg3_atomnas_a_shrink0.3.json 2> $OUT/${T}_bench_cfg3.err
timeout 400 python bench.py --full --model atomnas_c_plus --batch 128 --no-cpu-baseline > $OUT/${T}_bench_cfg5_atomnas_c_plus_bs128.json 2> $OUT/${T}_bench_cfg5.err
timeout 400 python bench.py --input-pipeline uint8 --no-cpu-baseline --no-roofline > $OUT/${T}_bench_input_pipeline_uint8.json 2> $OUT/${T}_bench_u8.err
timeout 400 python bench.py --no-cpu-baseline --no-roofline > $OUT/${T}_bench_resident_same_call.json 2> $OUT/${T}_bench_res.err
timeout 300 python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > $OUT/${T}_smoke.log 2>&1
timeout 900 python bench.py --full > $OUT/${T}_final_bench.json 2> $OUT/${T}_final_bench.err
rm -rf $OUT/prof_$T/*/*.db $OUT/pmc_$T 2>/dev/null   # the raw traces are large: only the summaries are kept
find $OUT/prof_$T -name "*kernel_trace.csv" -size +20M -delete 2>/dev/null
cat $OUT/${T}_pytest_full.log | tail -3; tail -2 $OUT/${T}_final_bench.err; cut -c1-420 $OUT/${T}_final_bench.json; tail -2 $OUT/${T}_smoke.log
for f in cfg2_atomnas_a_supernet cfg3_atomnas_a_shrink0.3 cfg5_atomnas_c_plus_bs128 input_pipeline_uint8 resident_same_call; do echo "$f: $(grep -o '"value": [0-9.]*' $OUT/${T}_bench_$f.json | head -1) $(grep -o '"ms_per_step": [0-9.]*' $OUT/${T}_bench_$f.json | head -1)"; done
cat $OUT/${T}_graph_gaps.txt | head -4
