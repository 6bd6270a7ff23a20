# Round-3 evidence run (one MI355X box): bash profiles/r03_profile_cmd.sh <tag>   -> gpurun_out/<tag>/..., summarised into profiles/ by
# profiles/summarize.py + profiles/tools/sq_counters.py (see profiles/README.md).  Every rocprofv3 command has the program itself behind "--";
# counters are collected in their own passes (--kernel-trace only).
set -x
TAG=${1:-r3}
R=$GRAFT_REPO_ROOT
O=$R/gpurun_out/$TAG
mkdir -p $O
python3 $R/bench.py --full --steps 200 --warmup 20 > $O/bench.json 2> $O/bench.err
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof -o p -- python3 $R/bench.py --full --steps 100 --warmup 10 --no-cpu-baseline --no-stress > $O/bench_under_prof.json 2> $O/prof_err.log
rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d $O/pmc_fetch -o f -- python3 $R/bench.py --full --steps 10 --warmup 3 --no-cpu-baseline --no-stress > $O/pmc_fetch.json 2> $O/pmc_fetch_err.log
rocprofv3 --kernel-trace --pmc WRITE_SIZE --output-format csv -d $O/pmc_write -o w -- python3 $R/bench.py --full --steps 10 --warmup 3 --no-cpu-baseline --no-stress > $O/pmc_write.json 2> $O/pmc_write_err.log
rocprofv3 --kernel-trace -d $O/tl -o tl -- python3 $R/bench.py --full --steps 60 --warmup 10 --no-cpu-baseline --no-stress > /dev/null 2>&1
cd $R
rm -f $O/prof/*kernel_trace.csv $O/pmc_*/*kernel_trace.csv
python3 profiles/tools/step_timeline.py $O/tl/tl_results.db > $O/step_timeline.txt 2>&1
rm -rf $O/tl
bash profiles/tools/sq_counters.sh $TAG > $O/sq.log 2>&1
python3 -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > $O/smoke.log 2>&1
for w in cfg5-uniform cfg5-real cfg4 cfg3 cfg1; do python3 bench.py --full --workload $w --no-cpu-baseline > $O/bench_$w.json 2> $O/bench_$w.err; done
python3 bench.py --full --model bert4rec --no-cpu-baseline > $O/bench_bert4rec.json 2> $O/bench_bert4rec.err
python3 bench.py --full --dtype bf16 --no-cpu-baseline > $O/bench_cfg2_bf16.json 2> $O/bench_cfg2_bf16.err
python3 bench.py --full --workload cfg3 --dtype bf16 --no-cpu-baseline > $O/bench_cfg3_bf16.json 2> $O/bench_cfg3_bf16.err
AMID_SEQ_FWD_VARIANT=1 python3 bench.py --full --no-cpu-baseline --no-stress > $O/bench_whole_row_forward.json 2> $O/bench_whole_row_forward.err
(echo "# python profiles/tools/variant_steps.py (cfg 2 shape: B 256, T 50, D 128, hid 32, neg 1; hipGraph replay, 200 steps)"; python3 profiles/tools/variant_steps.py 2>&1 | grep "ms/step"; echo "# VARIANT_T=20 (the mybank shape run.sh trains on)"; VARIANT_T=20 python3 profiles/tools/variant_steps.py 2>&1 | grep "ms/step"; echo "# python profiles/tools/cli_throughput.py --dr"; python3 profiles/tools/cli_throughput.py --dr 2>&1 | grep "samples/s") > $O/variant_steps.txt
python3 profiles/tools/dp_overhead.py 2>&1 | grep "ms/step" > $O/dp_overhead.txt
python3 profiles/tools/k1_time.py 2>&1 | grep "TB/s" > $O/k1_time.txt
python3 profiles/tools/seqn_stamps.py 2>&1 | grep -v amdgpu > $O/seqn_stamps.txt
# cfg 4 past its first epoch (480 batches): the lazy-Adam catch-up then replays 480-step gaps -- the default window (20 + 200 steps) never gets there
python3 bench.py --full --workload cfg4 --steps 480 --warmup 520 --no-cpu-baseline --no-stress > $O/bench_cfg4_steady.json 2> $O/bench_cfg4_steady.err
AMID_SEQ_BACKWARD=0 python3 bench.py --full --workload cfg4 --no-cpu-baseline --no-stress > $O/bench_cfg4_strip_backward.json 2> $O/bench_cfg4_strip_backward.err
python3 profiles/tools/seqn_bwd_stamps.py 2>&1 | grep -v amdgpu > $O/seqn_bwd_stamps.txt
python3 profiles/tools/probe/catchup_gap.py 2>&1 | grep "gap" > $O/catchup_gap.txt
(echo "# python profiles/tools/probe/d64_probe.py (B 256, T 50, synthetic batch; eager kernel list us/launches, then 200 replayed steps)"; python3 profiles/tools/probe/d64_probe.py 2>&1 | grep "D="; echo "# PROBE_D=128, the same script"; PROBE_D=128 python3 profiles/tools/probe/d64_probe.py 2>&1 | grep "D=") > $O/d64_probe.txt
ls -la $O
tail -3 $O/smoke.log
tail -c 400 $O/bench.json
