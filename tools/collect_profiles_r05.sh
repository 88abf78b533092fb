# Round-5 evidence: bench lines (headline, cfg 3 / 4 / 5, iter, fp32-MFMA), rocprofv3 kernel trace + stats, PMC passes (HBM traffic, MFMA /
# LDS counters), the training step, the fused level-0 block A/B, the evaluation driver with its loader threads.
# Run on the GPU box:  bash tools/collect_profiles_r05.sh      (writes gpurun_out/r05/, copy what is judged into profiles/)
set -x
R=$GRAFT_REPO_ROOT; O=$R/gpurun_out/r05; mkdir -p $O
cd $R
python bench.py --full --steps 20 --warmup 5 2>$O/once.err | tail -1 > $O/r05_bench_once.json
python bench.py --full --cfg 3 --steps 6 --warmup 2 2>/dev/null | tail -1 > $O/r05_bench_cfg3_sidd.json
python bench.py --full --steps 10 --warmup 3 --mode iter --no-cpu-baseline 2>/dev/null | tail -1 > $O/r05_bench_iter.json
python bench.py --full --steps 6 --warmup 2 --cfg 4 --no-cpu-baseline 2>/dev/null | tail -1 > $O/r05_bench_cfg4_unet_batch8.json
python bench.py --full --steps 6 --warmup 2 --cfg 5 --no-cpu-baseline 2>/dev/null | tail -1 > $O/r05_bench_cfg5_fp16.json
python bench.py --full --steps 6 --warmup 2 --precision fp32-mfma --no-cpu-baseline 2>/dev/null | tail -1 > $O/r05_bench_fp32_mfma.json
python tools/stage_bench.py > $O/r05_stage_kernels.txt 2>&1
python tools/layer_times.py > $O/r05_layer_times.txt 2>&1
python tools/layer_times.py 32 128 128 > $O/r05_layer_times_cfg3.txt 2>&1
python tools/block0_ab.py > $O/r05_block0_ab.txt 2>&1
python tools/train_bench.py --steps 30 > $O/r05_train_bench.txt 2>&1
python YOND_SIDD.py --synthetic 40 2>&1 | grep -E "images on|steady|Iter" > $O/r05_eval_driver_synthetic40.txt
cd /tmp && export TMPDIR=/tmp
B="python3 $R/bench.py --full --steps 2 --warmup 1 --frames-per-step 4 --no-cpu-baseline --no-extras --min-warmup-s 0"
rocprofv3 --kernel-trace --stats --output-format csv -d $O/trace -o t -- $B > /dev/null 2>&1
rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d $O/pmc_fetch -o f -- $B > /dev/null 2>&1
rocprofv3 --kernel-trace --pmc WRITE_SIZE --output-format csv -d $O/pmc_write -o w -- $B > /dev/null 2>&1
rocprofv3 --kernel-trace --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES SQ_INSTS_VALU_MFMA_MOPS_F16 SQ_WAVE_CYCLES --output-format csv -d $O/pmc_mfma -o m -- $B > /dev/null 2>&1
rocprofv3 --kernel-trace --stats --output-format csv -d $O/train_trace -o t -- python3 $R/tools/train_bench.py --steps 4 > $O/train_trace_bench.txt 2>&1
rocprofv3 --kernel-trace --output-format csv -d $O/frame_trace -o f -- python3 $R/tools/frame_trace.py > /dev/null 2>&1
cd $R
python tools/kmedians.py $O/trace > $O/r05_bench_once_kernel_medians.txt 2>&1
python tools/frame_trace_summary.py $O/frame_trace > $O/r05_frame_launches.txt 2>&1
cp $O/trace/t_kernel_stats.csv $O/r05_bench_once_kernel_stats.csv
cp $O/train_trace/t_kernel_stats.csv $O/r05_train_step_kernel_stats.csv
python tools/pmc_traffic.py $O/pmc_fetch $O/pmc_write $O/r05_pmc_traffic.json | head -40 > $O/r05_pmc_traffic_top.txt
python tools/pmc_kernel_means.py $O/pmc_mfma > $O/r05_pmc_mfma.txt 2>&1
rm -rf $O/pmc_fetch $O/pmc_write $O/pmc_mfma $O/frame_trace $O/trace/*trace* $O/train_trace/*trace* 2>/dev/null
ls -la $O
