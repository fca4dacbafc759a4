#!/bin/bash
# Round-4 evidence on the GPU box, everything from ONE build: kernel trace + stats and the counter passes of the bench command
# (tools/round_evidence.sh), the per-shape timing, the SE micro-benchmark and the kernel trace of config 5, smoke(), and last the
# default bench line (after the PMC summaries have been written to profiles/ with this build's source digest).
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$R/out}; mkdir -p "$OUT"; export OUT
cd $R
bash tools/round_evidence.sh r04
python tools/rocprof_summary.py $OUT/prof_r04/k_kernel_trace.csv > $OUT/r04_bench_bs256_kernel_summary.txt 2>&1
python tools/pmc_traffic.py $OUT/pmc_r04 > profiles/r04_pmc_traffic.json 2> $OUT/r04_pmc_traffic.log
python tools/pmc_mfma.py $OUT/pmc_r04/MFMA > profiles/r04_pmc_mfma.json 2> $OUT/r04_pmc_mfma.log
cp profiles/r04_pmc_traffic.json profiles/r04_pmc_mfma.json $OUT/ 2>/dev/null
DETAIL=1 timeout 300 python tools/bringup.py 256 > $OUT/r04_bs256_per_shape_timing.txt 2>&1
timeout 200 python tools/sebench.py > $OUT/r04_sebench.txt 2>&1
(cd /tmp && export TMPDIR=/tmp && timeout 400 rocprofv3 --kernel-trace --stats -d $OUT/prof_r04_cfg5 -o p --output-format csv -- python $R/bench.py --model atomnas_c_plus --batch 128 --steps 5 --warmup 2 --no-cpu-baseline --no-roofline > $OUT/prof_r04_cfg5.log 2>&1)
python tools/kstats.py $OUT/prof_r04_cfg5 > $OUT/r04_cfg5_kernel_summary.txt 2>&1
python tools/kstats.py $OUT/prof_r04_cfg5 k_se_ --launches > $OUT/r04_cfg5_se_kernels.txt 2>&1
timeout 300 python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > $OUT/r04_smoke.log 2>&1
timeout 900 python bench.py --full > $OUT/r04_final_bench.json 2> $OUT/r04_final_bench.err
tail -3 $OUT/r04_final_bench.err; cat $OUT/r04_final_bench.json | cut -c1-400; tail -2 $OUT/r04_smoke.log
