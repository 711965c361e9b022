#!/bin/bash
# Profiles of the C5 bench for profiles/ (run on the GPU box from the repo root):
#   kernel-trace stats, then separate PMC passes (FETCH_SIZE, WRITE_SIZE, SQ instruction mix / stalls).
#   usage: tools/profile_c5.sh OUTDIR
R=${GRAFT_REPO_ROOT:-$PWD}
mkdir -p "${1:?usage: tools/profile_c5.sh OUTDIR}" && O=$(cd "$1" && pwd)
cd /tmp && export TMPDIR=/tmp
# kernel-trace statistics: the bench command with everything --full measures (pre-warmed clocks, 20 timed steps);
# counter passes: a few dispatches are enough and the counters do not depend on the clock
rocprofv3 --kernel-trace --stats -d $O/prof_stats --output-format csv -- python3 $R/bench.py --gpus 1 --steps 20 --warmup 5 --full > $O/prof_stats.log 2>&1
# the TIMED launches alone (tools/rocprof_timed.py: dispatches [first_timed_step, first_timed_step + K) of each map kernel out of the
# trace of the --full command without the host-side extras) -> OUTDIR/r05_timed_launches.json (copy to profiles/)
rocprofv3 --kernel-trace --stats -d $O/prof_timed --output-format csv -- python3 $R/bench.py --gpus 1 --steps 20 --warmup 5 --full --no-cpu-baseline --no-optimize --no-other-configs --no-api > $O/prof_timed.log 2>&1
(cd $R && python3 tools/rocprof_timed.py $O/prof_timed $O/prof_timed.log --out $O/r05_timed_launches.json > $O/prof_timed_summary.txt 2>&1; find $O/prof_timed -name '*kernel_stats.csv' | head -1 | xargs -I{} cp {} $O/prof_timed_kernel_stats.csv; rm -rf $O/prof_timed)
# (--no-api: the pipelined host boundary launches the same kernels on chunks of rows - full-size launches only for the counters)
ARGS="--steps 5 --warmup 1 --prewarm-seconds 0 --full --no-cpu-baseline --no-optimize --no-other-configs --no-api"
rocprofv3 --kernel-trace --pmc FETCH_SIZE -d $O/prof_fetch --output-format csv -- python3 $R/bench.py $ARGS > $O/prof_fetch.log 2>&1
rocprofv3 --kernel-trace --pmc WRITE_SIZE -d $O/prof_write --output-format csv -- python3 $R/bench.py $ARGS > $O/prof_write.log 2>&1
rocprofv3 --kernel-trace --pmc SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_INSTS_SMEM -d $O/prof_sq --output-format csv -- python3 $R/bench.py $ARGS > $O/prof_sq.log 2>&1
cd $R
python3 tools/pmc_summary.py $O/prof_fetch $O/prof_write $O/prof_sq > $O/prof_pmc_summary.json
find $O/prof_stats -name '*kernel_stats.csv' | head -1 | xargs -I{} cp {} $O/prof_kernel_stats.csv
# (raw traces: hundreds of MB - the 2000 filter cycles alone are half a million dispatches; only the summaries are kept)
rm -rf $O/prof_stats $O/prof_fetch $O/prof_write $O/prof_sq
