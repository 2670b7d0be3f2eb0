#!/bin/bash
# The round's evidence bundle (run on the GPU box): GPU tests, kernel-trace + PMC traffic passes, per-kernel table, bench lines.
#   bash tools/evidence_bundle.sh OUT_DIR; then: python tools/collect_profiles.py r04 r04 OUT_DIR
# Every GPU step runs under a time limit of its own, and the first step that fails ends the script.
set -o pipefail
R=${GRAFT_REPO_ROOT:-/root/repo}
OUT=$(realpath -m "${1:?usage: bash tools/evidence_bundle.sh OUT_DIR}") && mkdir -p "$OUT" || exit 1
cd $R
(timeout -k 10 600 python -m pytest tests -m gpu -x -q > "$OUT/r4_tests.log" 2>&1; echo "rc=$?" >> "$OUT/r4_tests.log"; tail -3 "$OUT/r4_tests.log")
grep -q "rc=0" "$OUT/r4_tests.log" || exit 1
bash tools/profile_round.sh r04 "$OUT" || exit 1
echo profiled
cd $R && timeout -k 10 900 python tools/bench_kernels.py --gbuffer both --hzb --cull --post --iters 300 --cache "$OUT/urcache" > "$OUT/r4_kernels.txt" 2>&1 || exit 1
grep -v amdgpu.ids "$OUT/r4_kernels.txt"
timeout -k 10 600 python bench.py --full --steps 20 --warmup 5 > "$OUT/r4_b20.json" 2> "$OUT/r4_b20.err" || exit 1
tail -c 400 "$OUT/r4_b20.json"
for i in 1 2 3; do timeout -k 10 300 python bench.py --full --no-cpu-baseline --no-extras 2>/dev/null | python3 -c "import sys,json; d=json.loads(sys.stdin.read().strip().splitlines()[-1]); r=d['roofline']; print('bench1000', round(d['value']), 'frame_us', round(d['ms_per_step']*1e3,2), 'dispatch_us', round(r['avg_launch_us'],2), 'frac', round(r['frac'],4), 'alone', round(r['alone_on_stream_us'],2), 'n', r['launches_sampled'])" || exit 1; done | tee "$OUT/r4_bench_runs.txt" || exit 1
