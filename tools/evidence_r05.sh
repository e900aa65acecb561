#!/bin/bash
# GPU box: regenerate round 5's committed evidence under gpurun_out/ev5/ (copy into profiles/ afterwards).
#   tools/evidence_r05.sh [quick]      quick: skip the MPC / training / fuzz / drift legs
REPO=${GRAFT_REPO_ROOT:-/root/repo}; cd $REPO; EV=$REPO/gpurun_out/ev5; rm -rf $EV; mkdir -p $EV
python -c "import torch" 2>/dev/null
python bench.py --full --steps 20 --warmup 5 > $EV/r05_bench.json 2> $EV/bench.err
python bench.py --steps 5 --warmup 2 --streams 1 --full --no-cpu-baseline --no-extra > $EV/r05_bench_1stream.json 2>> $EV/bench.err
python bench.py --steps 5 --warmup 2 --streams 2 --full --no-cpu-baseline --no-extra > $EV/r05_bench_2streams.json 2>> $EV/bench.err
# BASELINE configs[3] at its global batch on one GPU (8 GPUs would take 64 graphs each)
python bench.py --material cloth --global-batch 512 --rollout-steps 20 --steps 3 --warmup 1 --full --no-cpu-baseline --no-extra > $EV/r05_bench_cloth512.json 2>> $EV/bench.err
python tools/fwd_err.py > $EV/r05_fwd_err.txt 2>/dev/null
python tools/dyn_err.py > $EV/r05_dyn_err.txt 2>/dev/null
if [ "$1" != "quick" ]; then
python tools/stress_repeat.py 300 > $EV/r05_stress_repeat.txt 2>/dev/null
python tools/fuzz_parity.py 5000 505 > $EV/r05_fuzz_parity.txt 2>/dev/null
# measured 10- / 20-step rollout drift per arithmetic mode at the three benchmarked shapes (one line per sample)
rm -f $EV/r05_rollout_drift.txt
AG_DRIFT_FILE=$EV/r05_rollout_drift.txt python -m pytest tests/test_gpu_parity.py -q -m gpu -k "test_rollout_at_the_benchmarked_config_vs_oracle" > $EV/drift_pytest.log 2>&1
{
echo "# bench_mpc.py on one MI355X (precision fast): BASELINE configs[4] and the reference planner's shipped shape (config/planning/rope.yaml:28-42)"
for args in "" "--particles 200 --samples 20000" "--particles 200 --samples 500"; do
  python bench_mpc.py --steps 3 --warmup 1 $args 2>> $EV/bench.err | tail -1
done
} > $EV/r05_mpc_bench.json
python bench_train.py --graph > $EV/r05_train_bench.json 2>> $EV/bench.err
fi
cd /tmp && export TMPDIR=/tmp
for m in "rope 256 10" "granular 128 10" "cloth 64 20"; do set -- $m
  rm -rf $EV/trace1
  timeout 300 rocprofv3 --kernel-trace --stats -d $EV/trace1 -o t -- python $REPO/bench.py --material $1 --batch $2 --rollout-steps $3 --steps 5 --warmup 2 --streams 1 --full --no-cpu-baseline --no-extra > $EV/r05_bench_1stream_traced_$1.json 2>/dev/null
  python $REPO/tools/rocpd_summary.py trace $(find $EV/trace1 -name "*.db" | head -1) > $EV/r05_kernel_trace_stats_1stream_$1.txt
done
rm -rf $EV/trace1
# edge encoder / node update: matrix-pipe busy fraction and clock (SQ counters, their own pass: no trace domains)
timeout 300 rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_INSTS_VALU GRBM_GUI_ACTIVE -d $EV/pmc_sq -o pmc -- \
   python $REPO/bench.py --steps 1 --warmup 1 --streams 1 --no-cpu-baseline --no-profile --no-extra > /dev/null 2>&1
python $REPO/tools/rocpd_summary.py pmc $(find $EV/pmc_sq -name "*.db" | head -1) > $EV/r05_sq_pmc.txt 2>/dev/null
rm -rf $EV/pmc_sq
timeout 1500 python $REPO/tools/pmc_traffic.py --out $EV/pmc_traffic.json > /dev/null 2>&1
# the bench line once more, now that the traffic file matches the sources being run (bench.py quotes it only then)
cp $EV/pmc_traffic.json $REPO/profiles/pmc_traffic.json
cd $REPO && python bench.py --full --steps 20 --warmup 5 > $EV/r05_bench.json 2>> $EV/bench.err
ls -la $EV
