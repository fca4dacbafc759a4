#!/bin/bash
# Refresh of the build-dependent evidence after the last kernel change of the round (the two-group instance of the depthwise backward on
# the matrix cores): the depthwise kernel tests, the kernel trace + PMC passes, the per-shape timing and the default bench line.
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$R/out}; mkdir -p "$OUT"; export OUT
cd $R
timeout 900 python -m pytest tests/test_kernels_gpu.py tests/test_block_gpu.py tests/test_parity_gpu.py -q -m gpu -k "dwconv or block or blockwise" 2>&1 | tail -4 > $OUT/r05b_pytest.log
rm -rf $OUT/prof_r05 $OUT/pmc_r05
bash tools/profile_round.sh r05 > $OUT/evidence_r05.log 2>&1
(cd /tmp && export TMPDIR=/tmp && timeout 600 rocprofv3 --kernel-trace --pmc SQ_INSTS_VALU_MFMA_MOPS_BF16 SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES --output-format csv -d $OUT/pmc_r05/MFMA -o p -- python $R/bench.py --steps 2 --warmup 1 --no-cpu-baseline --no-roofline > $OUT/pmc_r05_MFMA.log 2>&1)
python tools/rocprof_summary.py $OUT/prof_r05/k_kernel_trace.csv > $OUT/r05_bench_bs256_kernel_summary.txt 2>&1
python tools/pmc_traffic.py $OUT/pmc_r05 > profiles/r05_pmc_traffic.json 2> $OUT/r05_pmc_traffic.log
python tools/pmc_mfma.py $OUT/pmc_r05/MFMA > profiles/r05_pmc_mfma.json 2> $OUT/r05_pmc_mfma.log
cp profiles/r05_pmc_traffic.json profiles/r05_pmc_mfma.json $OUT/ 2>/dev/null
DETAIL=1 timeout 300 python tools/bringup.py 256 > $OUT/r05_bs256_per_shape_timing.txt 2>&1
timeout 900 python bench.py --full > $OUT/r05_final_bench.json 2> $OUT/r05_final_bench.err
cat $OUT/r05b_pytest.log | tail -2; tail -1 $OUT/r05_final_bench.err; cut -c1-300 $OUT/r05_final_bench.json
