#!/bin/bash
# Refresh the judged artefacts of a round (run on the GPU box through gpurun from the repository root):
#   bench lines (headline as the driver runs it, the other workloads, the observation sink), kernel-trace stats of the bench
#   command with the default two chains and with one chain (per-kernel durations do not overlap), the GPU test suite with the
#   parity log.  Counter passes: tools/profiling/pmc_r2.sh (separate call).  Copy what should be judged from gpurun_out/ to profiles/.
R=$GRAFT_REPO_ROOT; out=$R/gpurun_out/prof_r2; rm -rf $out; mkdir -p $out
cd $R
rm -f gpurun_out/r2_parity.json
timeout 900 python -m pytest tests -m gpu -q > $out/pytest.log 2>&1; echo "pytest rc $?" >> $out/pytest.log; tail -3 $out/pytest.log
cp gpurun_out/r2_parity.json $out/r2_parity.json
timeout 400 python bench.py --gpus 1 --steps 20 --warmup 5 --full > $out/bench_sloth_32env.json 2> $out/bench.err; tail -c 600 $out/bench_sloth_32env.json; echo
: > $out/bench_other_configs.jsonl
for cfg in rope_1env T_32env T_pusher_32env sloth_multicam_8env; do
  timeout 300 python bench.py --config $cfg --steps 20 --warmup 5 --full --no-cpu-baseline 2>/dev/null | tail -1 >> $out/bench_other_configs.jsonl
done
timeout 300 python bench.py --steps 20 --warmup 5 --full --no-cpu-baseline --sink /tmp/r2_sink 2>/dev/null | tail -1 >> $out/bench_other_configs.jsonl
python - <<'PY'
import json
for l in open('gpurun_out/prof_r2/bench_other_configs.jsonl'):
    d = json.loads(l); print(d['config']['workload'][:60], round(d['value'], 1), {k: (round(v['ms_per_step'], 2), v['mesh_contacts'], v['self_collision_candidates']) for k, v in d['phases'].items() if isinstance(v, dict)}, d.get('observation_sink'))
PY
cd /tmp && export TMPDIR=/tmp
for mode in default chains1; do
  if [ $mode = chains1 ]; then export R2S_CHAINS=1; else unset R2S_CHAINS; fi
  timeout 400 rocprofv3 --kernel-trace --stats -d $out/trace_$mode -o bench -- python $R/bench.py --steps 6 --warmup 3 --full --no-cpu-baseline > $out/bench_trace_$mode.log 2>&1 || echo trace-failed
  db=$(find $out/trace_$mode -name "*.db" | head -1)
  python $R/tools/rocpd_stats.py $db $out/kernel_stats_$mode.md > /dev/null 2>&1 || echo stats-failed
  head -9 $out/kernel_stats_$mode.md | cut -c1-70,150-240
  rm -rf $out/trace_$mode
done
unset R2S_CHAINS
# the large-mesh finishing kernel (k_contact_finish<2>) in its own table: the pusher workload, second half of the window in contact
timeout 400 rocprofv3 --kernel-trace --stats -d $out/trace_pusher -o bench -- python $R/bench.py --config T_pusher_32env --steps 6 --warmup 3 --full --no-cpu-baseline > $out/bench_trace_pusher.log 2>&1 || echo trace-failed
db=$(find $out/trace_pusher -name "*.db" | head -1)
python $R/tools/rocpd_stats.py $db $out/kernel_stats_pusher.md > /dev/null 2>&1 || echo stats-failed
head -6 $out/kernel_stats_pusher.md | cut -c1-70,150-240
rm -rf $out/trace_pusher
