#!/bin/bash
# End-of-round checks on an MI355X host: the whole `-m gpu` suite, __graft_entry__.smoke(), the full bench record and the
# rocprofv3 kernel-trace summary of the bench command; everything lands under the directory given (default: final_checks/).
#   bash scripts/run_final_checks.sh [out_dir]
set -u
OUT=${1:-final_checks}
mkdir -p $OUT
export EGX_P3_TABLE=$PWD/$OUT/p3_table.txt EGX_C5_HIST=$PWD/$OUT/c5_hist.txt EGX_TOL_REPORT=$PWD/$OUT/env_tolerance_usage.txt
rm -f $EGX_P3_TABLE $EGX_TOL_REPORT
EGX_DRIFT_TABLE=$OUT/drift_table.txt timeout 3000 python -m pytest tests -x -q -m gpu < /dev/null > $OUT/gpu_tests.log 2>&1
echo "gpu tests rc=$?"; tail -4 $OUT/gpu_tests.log
timeout 300 python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" < /dev/null > $OUT/smoke.log 2>&1
echo "smoke rc=$?"; tail -2 $OUT/smoke.log
timeout 1500 python bench.py --gpus 1 --steps 20 --warmup 5 --full --extra-configs 2 --detail-file $PWD/$OUT/bench_detail.json < /dev/null > $OUT/bench.json 2> $OUT/bench.err
echo "bench rc=$?"; cut -c1-300 $OUT/bench.json
bash scripts/run_profile.sh final > $OUT/profile.log 2>&1
tail -3 $OUT/profile.log
PMC_SETS="FETCH_SIZE WRITE_SIZE TCC_HIT_sum,TCC_MISS_sum GRBM_GUI_ACTIVE,SQ_BUSY_CU_CYCLES SQ_VALU_MFMA_BUSY_CYCLES,SQ_INSTS_VALU_MFMA_MOPS_F16 TCP_TCC_READ_REQ_sum,TCP_TOTAL_CACHE_ACCESSES_sum SQ_ACTIVE_INST_VALU,SQ_INSTS_VALU" bash scripts/pmc_lbs.sh final_pmc > $OUT/pmc.log 2>&1
tail -12 $OUT/pmc.log
