#!/bin/bash
# Round-5 evidence for profiles/: the bench line, rocprofv3 kernel stats of the bench command and of the production forward alone, HBM /
# SQ counters of the edge-group NNConv and the GIN pair (separate --pmc passes, kernel-trace only, every profiler command under its own
# timeout), HBM bytes of the whole forward per kernel, timelines (100 000 and 10 000 nodes), mid sizes, config 3, the sharded step at
# world 1.  Output: gpurun_out/r05/ (copied to profiles/r05_*).  The studies of the round have their own scripts (profiles/README.md).
cd $GRAFT_REPO_ROOT; export TMPDIR=/tmp
O=gpurun_out/r05; mkdir -p $O
timeout 900 python bench.py --full > $O/bench.json 2> $O/bench.err
rm -rf /tmp/r05_ks; timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/r05_ks -- python bench.py --full --steps 10 --warmup 3 --no-cpu-baseline --no-train-step --no-extra-sizes > /tmp/r05_ks.log 2>&1
f=$(find /tmp/r05_ks -name "*kernel_stats.csv" | head -1); [ -n "$f" ] && { cp $f $O/kernel_stats.csv; python scratch/kstats.py $f 30 > $O/kernel_stats_summary.txt; }
rm -rf /tmp/r05_fw; timeout 300 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/r05_fw -- python scratch/run_fwd_mode.py 1 20 > /tmp/r05_fw.log 2>&1
python scratch/kstats.py $(find /tmp/r05_fw -name "*kernel_stats.csv" | head -1) 26 > $O/forward_kernel_stats.txt
timeout 200 python scratch/run_stamped.py > $O/stamped_nnconv.txt 2>&1
: > $O/pmc_nnconv.txt
i=0
for grp in "FETCH_SIZE" "WRITE_SIZE" \
           "SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_BUSY_CYCLES SQ_WAVES" \
           "SQ_INSTS_VALU SQ_INSTS_VMEM SQ_INSTS_LDS SQ_INSTS_MFMA SQ_INSTS_SALU SQ_INSTS_BRANCH SQ_VALU_MFMA_BUSY_CYCLES" ; do
  i=$((i+1)); rm -rf /tmp/pmc_r05_$i
  timeout 200 rocprofv3 --kernel-trace --pmc $grp --output-format csv -d /tmp/pmc_r05_$i -- python scratch/run_nnconv_only.py nnconv > /tmp/pmc_r05_$i.log 2>&1
  f=$(find /tmp/pmc_r05_$i -name "*counter_collection.csv" | head -1)
  [ -n "$f" ] && python scratch/pmc.py nnconv32_eg $f >> $O/pmc_nnconv.txt
done
for grp in "FETCH_SIZE" "WRITE_SIZE"; do
  rm -rf /tmp/pmc_r05_g
  timeout 200 rocprofv3 --kernel-trace --pmc $grp --output-format csv -d /tmp/pmc_r05_g -- python scratch/run_nnconv_only.py gin > /tmp/pmc_r05_g.log 2>&1
  f=$(find /tmp/pmc_r05_g -name "*counter_collection.csv" | head -1)
  [ -n "$f" ] && { python scratch/pmc.py gin32_aggregate $f | sed 's/^/gin32_aggregate /'; python scratch/pmc.py gin32_mlp $f | sed 's/^/gin32_mlp /'; } >> $O/pmc_nnconv.txt
done
bash scratch/pmc_forward.sh > $O/pmc_forward.txt 2>&1
bash scratch/mid_trace.sh 100000 > /dev/null 2>&1; cp gpurun_out/mid_trace_100000/timeline.txt $O/trace_100000.txt
bash scratch/mid_trace.sh 10000 > /dev/null 2>&1; cp gpurun_out/mid_trace_10000/timeline.txt $O/mid_trace_10000.txt
timeout 300 python scratch/time_mid.py > $O/mid_sizes.txt 2>&1
bash scratch/kstats3.sh r05_config3 > $O/config3_kernel_stats.txt 2>&1
timeout 200 python scratch/time_config3.py 2>&1 | grep bfloat16 >> $O/config3_kernel_stats.txt
MASTER_ADDR=127.0.0.1 MASTER_PORT=29577 RANK=0 WORLD_SIZE=1 LOCAL_RANK=0 timeout 400 python bench.py --full --force-sharded --steps 20 --warmup 5 2>/dev/null | tail -1 > $O/bench_sharded_world1.json
ls -la $O
