#!/bin/bash
# Round-4 evidence run (one MI355X box): bash profiles/r04_profile_cmd.sh <tag>   -> gpurun_out/<tag>/..., summarised into profiles/ by
# profiles/collect_r04.sh (see profiles/README.md).  Every rocprofv3 command has the program itself behind "--"; counters are collected
# in their own passes (--kernel-trace only).
set -uo pipefail
set -x
TAG=${1:-r4}
R=${GRAFT_REPO_ROOT:-$(cd "$(dirname "$0")/.." && pwd)}
O=$R/gpurun_out/$TAG
mkdir -p "$O"
cd "$R"
# the driver's own command line, then the default one
python3 bench.py --full --steps 20 --warmup 5 > $O/bench_driver_args.json 2> $O/bench_driver_args.err
python3 bench.py --full --steps 200 --warmup 20 > $O/bench.json 2> $O/bench.err
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof -o p -- python3 $R/bench.py --full --steps 100 --warmup 10 --no-cpu-baseline --no-stress > $O/bench_under_prof.json 2> $O/prof_err.log
rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d $O/pmc_fetch -o f -- python3 $R/bench.py --full --steps 10 --warmup 3 --no-cpu-baseline --no-stress > $O/pmc_fetch.json 2> $O/pmc_fetch_err.log
rocprofv3 --kernel-trace --pmc WRITE_SIZE --output-format csv -d $O/pmc_write -o w -- python3 $R/bench.py --full --steps 10 --warmup 3 --no-cpu-baseline --no-stress > $O/pmc_write.json 2> $O/pmc_write_err.log
rocprofv3 --kernel-trace -d $O/tl -o tl -- python3 $R/bench.py --full --steps 60 --warmup 10 --no-cpu-baseline --no-stress > /dev/null 2>&1
rocprofv3 --kernel-trace -d $O/tlb -o tl -- python3 $R/bench.py --full --model bert4rec --steps 60 --warmup 10 --no-cpu-baseline --no-stress > /dev/null 2>&1
rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_bert -o p -- python3 $R/bench.py --full --model bert4rec --steps 100 --warmup 10 --no-cpu-baseline --no-stress > $O/bench_bert_under_prof.json 2> $O/prof_bert_err.log
cd "$R"
rm -f $O/prof/*kernel_trace.csv $O/pmc_*/*kernel_trace.csv $O/prof_bert/*kernel_trace.csv
python3 profiles/tools/step_timeline.py $O/tl/tl_results.db > $O/step_timeline.txt 2>&1
python3 profiles/tools/step_timeline.py $O/tlb/tl_results.db > $O/bert_step_timeline.txt 2>&1
rm -rf $O/tl $O/tlb
python3 -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > $O/smoke.log 2>&1
for w in cfg5-uniform cfg5-real cfg4 cfg3 cfg1; do python3 bench.py --full --workload $w --no-cpu-baseline > $O/bench_$w.json 2> $O/bench_$w.err; done
python3 bench.py --full --model bert4rec --no-cpu-baseline > $O/bench_bert4rec.json 2> $O/bench_bert4rec.err
python3 bench.py --full --dtype bf16 --no-cpu-baseline > $O/bench_cfg2_bf16.json 2> $O/bench_cfg2_bf16.err
python3 bench.py --full --workload cfg3 --dtype bf16 --no-cpu-baseline > $O/bench_cfg3_bf16.json 2> $O/bench_cfg3_bf16.err
# A/B on this box: the weight gradients on the fp32 matrix instructions (round 3's kernels)
AMID_WGRAD_SPLIT=0 python3 bench.py --full --no-cpu-baseline --no-stress > $O/bench_fp32_wgrad.json 2> $O/bench_fp32_wgrad.err
AMID_WGRAD_SPLIT=0 python3 bench.py --full --model bert4rec --no-cpu-baseline --no-stress > $O/bench_bert4rec_fp32_wgrad.json 2> $O/bench_bert4rec_fp32_wgrad.err
AMID_FOLD_CATCHUP=1 python3 bench.py --full --no-cpu-baseline --no-stress > $O/bench_fold_catchup.json 2> $O/bench_fold_catchup.err
python3 profiles/tools/probe/wgrad_split_probe.py 2>&1 | grep -v amdgpu > $O/wgrad_split_probe.txt
(echo "# python profiles/tools/variant_steps.py (cfg 2 shape: B 256, T 50, D 128, hid 32, neg 1; hipGraph replay, 200 steps)"; python3 profiles/tools/variant_steps.py 2>&1 | grep "ms/step"; echo "# VARIANT_T=20 (the mybank shape run.sh trains on)"; VARIANT_T=20 python3 profiles/tools/variant_steps.py 2>&1 | grep "ms/step") > $O/variant_steps.txt
(echo "# VARIANT_KERNELS=1 python profiles/tools/variant_steps.py: every variant's eager step, entry point by entry point (us per step / launches)"; VARIANT_KERNELS=1 python3 profiles/tools/variant_steps.py 2>&1 | grep -E "^  |ms/step") > $O/variant_kernels.txt
# A/B on this box: the forward's / the backward strips' products on the fp32 matrix instructions (round 3's kernels)
AMID_FWD_SPLIT=0 python3 bench.py --full --no-cpu-baseline --no-stress > $O/bench_fp32_forward.json 2> $O/bench_fp32_forward.err
AMID_BWD_SPLIT=0 python3 bench.py --full --no-cpu-baseline --no-stress > $O/bench_fp32_bwd_strips.json 2> $O/bench_fp32_bwd_strips.err
AMID_FWD_SPLIT=0 AMID_BWD_SPLIT=0 AMID_WGRAD_SPLIT=0 python3 bench.py --full --no-cpu-baseline --no-stress > $O/bench_fp32_everything.json 2> $O/bench_fp32_everything.err
python3 profiles/tools/dp_overhead.py 2>&1 | grep "ms/step" > $O/dp_overhead.txt
python3 profiles/tools/k1_time.py 2>&1 | grep "TB/s" > $O/k1_time.txt
python3 profiles/tools/seqn_stamps.py 2>&1 | grep -v amdgpu > $O/seqn_stamps.txt
(echo "# AMID_FWD_SPLIT=0: the fp32 build (seqn_fwd_kernel)"; AMID_FWD_SPLIT=0 python3 profiles/tools/seqn_stamps.py 2>&1 | grep -v amdgpu) >> $O/seqn_stamps.txt
python3 profiles/tools/strip_bwd_stamps.py 2>&1 | grep -v amdgpu > $O/strip_bwd_stamps.txt
python3 bench.py --full --workload cfg4 --steps 480 --warmup 520 --no-cpu-baseline --no-stress > $O/bench_cfg4_steady.json 2> $O/bench_cfg4_steady.err
ls -la $O
tail -3 $O/smoke.log
tail -c 600 $O/bench_driver_args.json
