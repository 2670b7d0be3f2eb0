#!/bin/bash
# Round profile bundle (run on the GPU box): kernel-trace stats and the HBM-traffic PMC passes of `bench.py`.
#   bash tools/profile_round.sh r02 OUT_DIR  -> OUT_DIR/prof_r02_{trace,fetch,write}; each pass has a time limit, the first failure ends it
tag=${1:-rXX}
R=${GRAFT_REPO_ROOT:-/root/repo}
P=$(realpath -m "${2:?usage: bash tools/profile_round.sh TAG OUT_DIR}") && mkdir -p "$P" || exit 1
cd /tmp && export TMPDIR=/tmp
B="python3 $R/bench.py --full --steps 300 --warmup 200 --no-cpu-baseline --no-extras"
# the kernel-trace pass runs 4000 timed frames: the profiler averages over EVERY dispatch, the ~400 of the clock ramp (80+ us each) included,
# and with 300 timed frames those were a fifth of the sample (73.0 us against 71.4 in the steady part of the same trace)
BT="python3 $R/bench.py --full --steps 4000 --warmup 200 --no-cpu-baseline --no-extras"
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d "$P/prof_${tag}_trace" -- $BT > "$P/prof_${tag}_trace.log" 2>&1 || exit 1
timeout -k 10 300 rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d "$P/prof_${tag}_fetch" -- $B > "$P/prof_${tag}_fetch.log" 2>&1 || exit 1
timeout -k 10 300 rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d "$P/prof_${tag}_write" -- $B > "$P/prof_${tag}_write.log" 2>&1 || exit 1
