# Round-4 measurement set, all on ONE box so that the numbers agree with each other:
#   1. rocprofv3 --kernel-trace --stats of the bench command (fp32)   -> r04_kernel_by_grid.txt, r04_last_step_by_grid.txt (one replayed step) (+ rocprofv3's own kernel_stats CSV)
#   2. the same for --dtype bf16                                       -> r04_bf16_kernel_by_grid.txt
#   3. step-level PMC passes (eager step), fp32 and bf16                -> r04_pmc/hbm_traffic.json, hbm_traffic_bf16.json
#   4. fused residual-block kernels: phase stamps, per-level chain times, whole-step A/B (fused vs one kernel per op)
#   5. python bench.py --full (reads 1-3)                               -> r04_bench_n1.json ; smoke()
# Everything lands in gpurun_out/final4/ (the box's profiles/ does not travel back); copy the summaries to profiles/ afterwards.
set -x
cd $GRAFT_REPO_ROOT
export TMPDIR=/tmp
OUT=gpurun_out/final4
mkdir -p $OUT profiles/r04_pmc gpurun_out/r04
bash tools/r04_prof.sh f32 || exit 1
cp gpurun_out/r04/f32_kernel_by_grid.txt $OUT/r04_kernel_by_grid.txt; cp gpurun_out/r04/f32_kernel_stats.csv $OUT/r04_kernel_stats.csv
bash tools/r04_prof.sh bf16 --dtype bf16 || exit 1
cp gpurun_out/r04/bf16_kernel_by_grid.txt $OUT/r04_bf16_kernel_by_grid.txt
cp gpurun_out/r04/f32_last_step_by_grid.txt $OUT/r04_last_step_by_grid.txt; cp gpurun_out/r04/bf16_last_step_by_grid.txt $OUT/r04_bf16_last_step_by_grid.txt
bash tools/r04_pmc_step.sh f32 > $OUT/pmc_f32.log 2>&1 || { echo "PMC passes (fp32) failed"; tail -5 $OUT/pmc_f32.log; exit 1; }
N=$(grep steps_in_run $OUT/pmc_f32.log | cut -d= -f2)
python tools/pmc_step_json.py gpurun_out/r04_pmc_f32_f/f_counter_collection.csv gpurun_out/r04_pmc_f32_w/w_counter_collection.csv $N $OUT/hbm_traffic.json > $OUT/pmc_summary_f32.txt || exit 1
bash tools/r04_pmc_step.sh bf16 --dtype bf16 > $OUT/pmc_bf16.log 2>&1 || { echo "PMC passes (bf16) failed"; tail -5 $OUT/pmc_bf16.log; exit 1; }
N=$(grep steps_in_run $OUT/pmc_bf16.log | cut -d= -f2)
python tools/pmc_step_json.py gpurun_out/r04_pmc_bf16_f/f_counter_collection.csv gpurun_out/r04_pmc_bf16_w/w_counter_collection.csv $N $OUT/hbm_traffic_bf16.json 57.96e6 > $OUT/pmc_summary_bf16.txt || exit 1
rm -rf gpurun_out/r04_pmc_f32_f gpurun_out/r04_pmc_f32_w gpurun_out/r04_pmc_bf16_f gpurun_out/r04_pmc_bf16_w
cp $OUT/r04_kernel_by_grid.txt $OUT/r04_bf16_kernel_by_grid.txt $OUT/r04_kernel_stats.csv profiles/
cp $OUT/hbm_traffic.json $OUT/hbm_traffic_bf16.json profiles/r04_pmc/
bash tools/rb_stamps.sh > $OUT/r04_rb_stamps.txt 2>&1
python tools/rb_bench.py 2>&1 | grep -v amdgpu.ids > $OUT/r04_rb_chain_times.txt
python tools/launch_floor.py 2>&1 | grep -v amdgpu.ids > $OUT/r04_launch_floor.txt
bash tools/rb_step_ab.sh > $OUT/r04_rb_step_ab.txt 2>&1
bash tools/rb_step_ab.sh --dtype bf16 > $OUT/r04_rb_step_ab_bf16.txt 2>&1
python bench.py --full > $OUT/r04_bench_n1.json 2> $OUT/bench.err || exit 1
cut -c1-600 $OUT/r04_bench_n1.json
python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" 2>&1 | tail -2
cat $OUT/pmc_summary_f32.txt | head -12; cat $OUT/pmc_summary_bf16.txt | head -8; cat $OUT/r04_rb_step_ab.txt $OUT/r04_rb_step_ab_bf16.txt
