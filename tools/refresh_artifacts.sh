#!/bin/bash
# One pass over everything under profiles/ that a kernel change can move (run on the GPU box from the repo root; ~6 min):
#   tools/refresh_artifacts.sh r06      -> gpurun_out/refresh/r06_*   (copy what should be kept into profiles/)
set -x
R=${1:-r06}
cd $GRAFT_REPO_ROOT
O=$GRAFT_REPO_ROOT/gpurun_out/refresh
mkdir -p $O
python bench.py --full > $O/${R}_bench_default.json 2> $O/bench.err
tail -c 700 $O/${R}_bench_default.json
python bench.py --full --gemm-precision bf16s --no-cpu-baseline > $O/${R}_bench_bf16s.json 2>/dev/null; tail -c 400 $O/${R}_bench_bf16s.json
python bench.py --full --gemm-precision bf16 --no-cpu-baseline > $O/${R}_bench_bf16_operand_mode.json 2>/dev/null; tail -c 400 $O/${R}_bench_bf16_operand_mode.json
python bench.py --full --gemm-precision fp32x3 --no-cpu-baseline > $O/${R}_bench_fp32x3.json 2>/dev/null; tail -c 400 $O/${R}_bench_fp32x3.json
python tools/measure_protocol.py > $O/${R}_timing_protocol.json 2> $O/protocol.err; tail -c 400 $O/${R}_timing_protocol.json
python tools/named_configs.py > $O/${R}_named_configs.jsonl 2> $O/named.err; cut -c 1-300 $O/${R}_named_configs.jsonl
python tools/named_configs.py --precision bf16 >> $O/${R}_named_configs.jsonl 2>> $O/named.err
python tools/named_configs.py --precision fp32 >> $O/${R}_named_configs.jsonl 2>> $O/named.err
python tools/named_configs.py --precision fp32x3 >> $O/${R}_named_configs.jsonl 2>> $O/named.err
python tools/touch_bench.py > $O/${R}_touch_topology_step.log 2>&1; tail -3 $O/${R}_touch_topology_step.log
python tools/touch_bench.py --precision fp32x3 2>/dev/null | tail -1 >> $O/${R}_touch_topology_step.log
(cd /tmp && export TMPDIR=/tmp && rm -rf /tmp/bstats && rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/bstats -- python $GRAFT_REPO_ROOT/bench.py --steps 15 --warmup 5 --no-cpu-baseline --no-traffic --alt-steps 0 > /tmp/bstats.log 2>&1; cp $(find /tmp/bstats -name '*kernel_stats.csv' | head -1) $O/${R}_bench_kernel_stats.csv; tail -c 300 /tmp/bstats.log)
(cd /tmp && export TMPDIR=/tmp && rm -rf /tmp/bstats2 && rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/bstats2 -- python $GRAFT_REPO_ROOT/bench.py --steps 15 --warmup 5 --no-cpu-baseline --no-traffic --gemm-precision bf16s > /tmp/bstats2.log 2>&1; cp $(find /tmp/bstats2 -name '*kernel_stats.csv' | head -1) $O/${R}_bench_bf16s_kernel_stats.csv)
(cd /tmp && export TMPDIR=/tmp && rm -rf /tmp/bstats3 && rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/bstats3 -- python $GRAFT_REPO_ROOT/bench.py --steps 15 --warmup 5 --no-cpu-baseline --no-traffic --alt-steps 0 --gemm-precision fp32x3 > /tmp/bstats3.log 2>&1; cp $(find /tmp/bstats3 -name '*kernel_stats.csv' | head -1) $O/${R}_bench_fp32x3_kernel_stats.csv)
# round 6, bf16 configurations: the fused BatchNorm + ReLU operator and the 5 x 5 convolutions against MIOpen's per map shape
python tools/bnrelu_bench.py > $O/${R}_bnrelu_vs_miopen.txt 2>/dev/null
python tools/conv5_bench.py > $O/${R}_conv5_vs_miopen.txt 2>/dev/null; tail -2 $O/${R}_conv5_vs_miopen.txt
(./tools/ubench/mfma_plus_valu; ./tools/ubench/mfma_gap_budget; ./tools/ubench/mfma_one_wave) > $O/${R}_fp32_pipe_ubench.txt 2>&1
# error table of the gemm modes against the fp64 oracle
python -m pytest tests/test_gpu_fullsize.py -q -s -k benchmark_configuration 2>&1 | grep "^\[configs\|passed\|failed" > $O/${R}_mode_error_table.txt; cat $O/${R}_mode_error_table.txt
python -m pytest tests/test_gpu_fp32x3.py -q -s -k vs_fp64 2>&1 | grep "^\[\|passed\|failed" >> $O/${R}_mode_error_table.txt
# configs[3]: the first steps run MIOpen's find mode, so the table is cut from the kernel TRACE after 5 steps (tools/trace_steady.py)
(cd /tmp && export TMPDIR=/tmp && rm -rf /tmp/c3 && rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/c3 -- python $GRAFT_REPO_ROOT/tools/named_configs.py --only 3 --steps 10 > /tmp/c3.log 2>&1; python $GRAFT_REPO_ROOT/tools/trace_steady.py $(find /tmp/c3 -name "*kernel_trace.csv" | head -1) --marker chamfer_bwd --skip 5 --top 70 > $O/${R}_config3_bf16s_steady_kernels.txt; head -8 $O/${R}_config3_bf16s_steady_kernels.txt)
# the exact search: both geometries ("bench" = the untrained network's concentric sphere / ellipsoids), its work counters
(python tools/chamfer_bench.py --geometry bench; python tools/chamfer_bench.py) > $O/${R}_chamfer_search.txt 2>/dev/null; cat $O/${R}_chamfer_search.txt
(python tools/nn_stats.py --geometry bench; python tools/nn_stats.py; python tools/nn_stats_config.py --which 3 --batch 16 | tail -1; python tools/nn_stats_config.py --which 4 | tail -1) > $O/${R}_nn_pruning_stats.txt 2>/dev/null
python tools/score_bench.py 2>/dev/null | tail -1 > $O/${R}_scoring_batched_vs_sequential.json; cut -c 1-400 $O/${R}_scoring_batched_vs_sequential.json
python tools/host_bound.py 2>/dev/null | tail -2 > $O/${R}_named_configs_host_time.txt
bash tools/collect_nn.sh > $O/nn.log 2>&1; cp gpurun_out/nn/summary.json $O/${R}_pmc_nn_summary.json
bash tools/collect_traffic.sh > $O/traffic.log 2>&1; cp gpurun_out/traffic/summary.json $O/${R}_pmc_traffic_summary.json
bash tools/collect_sq.sh > $O/sq.log 2>&1; cp gpurun_out/sq/summary.json $O/${R}_pmc_sq_summary.json
bash tools/collect_sq.sh --precision bf16s > $O/sq16.log 2>&1; cp gpurun_out/sq/summary.json $O/${R}_pmc_sq_summary_bf16s.json
bash tools/collect_traffic.sh --precision fp32x3 > $O/traffic3.log 2>&1; cp gpurun_out/traffic/summary.json $O/${R}_pmc_traffic_summary_fp32x3.json
bash tools/collect_sq.sh --precision fp32x3 > $O/sq3.log 2>&1; cp gpurun_out/sq/summary.json $O/${R}_pmc_sq_summary_fp32x3.json
python -m torch.distributed.run --nnodes=1 --nproc-per-node 1 --master-addr 127.0.0.1 --master-port 29511 bench.py --gpus 1 --steps 5 --warmup 2 --no-cpu-baseline --no-traffic 2>/dev/null | tail -c 400
python tools/kstats_summary.py $O/${R}_bench_kernel_stats.csv 22 16
python tools/kstats_summary.py $O/${R}_bench_bf16s_kernel_stats.csv 22 12
python tools/kstats_summary.py $O/${R}_bench_fp32x3_kernel_stats.csv 22 14
