# Round-2 evidence run (one MI355X box): bash profiles/r02_profile_cmd.sh <tag>   -> gpurun_out/<tag>/..., summarised into profiles/ by
# profiles/summarize.py (see profiles/README.md).  Every rocprofv3 command has the program itself behind "--".
set -x
TAG=${1:-r2}
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
python3 -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > $O/smoke.log 2>&1
for w in cfg5-uniform cfg5-real cfg4 cfg3; do python3 bench.py --full --workload $w --no-cpu-baseline > $O/bench_$w.json 2> $O/bench_$w.err; done
python3 bench.py --full --model bert4rec --no-cpu-baseline > $O/bench_bert4rec.json 2> $O/bench_bert4rec.err
python3 bench.py --full --dtype bf16 --no-cpu-baseline > $O/bench_cfg2_bf16.json 2> $O/bench_cfg2_bf16.err
python3 bench.py --full --workload cfg3 --dtype bf16 --no-cpu-baseline > $O/bench_cfg3_bf16.json 2> $O/bench_cfg3_bf16.err
python3 profiles/tools/dp_overhead.py 2>&1 | grep "ms/step" > $O/dp_overhead.txt
python3 profiles/tools/k1_time.py 2>&1 | grep "TB/s" > $O/k1_time.txt
python3 profiles/tools/sort_time.py 2>&1 | grep -v amdgpu > $O/sort_time.txt
ls -la $O $O/*
tail -3 $O/smoke.log
tail -c 400 $O/bench.json
