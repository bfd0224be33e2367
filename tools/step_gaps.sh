#!/bin/bash
# GPU timeline of one train step from a rocprofv3 kernel trace: per kernel, mean duration and mean idle gap before it.
# Usage: bash tools/step_gaps.sh <workload> <tag> [extra bench args]   -> $OUT/<tag>_step_gaps.txt (OUT: profile_out)
set -e
WL=$1; TAG=$2; shift 2
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
OUT=${OUT:-profile_out}; mkdir -p "$OUT"
rm -rf "$OUT/_gt"
rocprofv3 --kernel-trace --output-format csv -d "$OUT/_gt" -o k -- python3 bench.py --full --workload $WL --steps 30 --warmup 5 --no-cpu-baseline --no-other-workloads --no-kernel-timers "$@" > "$OUT/${TAG}_gt.json" 2> "$OUT/${TAG}_gt.err"
F=$(find "$OUT/_gt" -name "*kernel_trace.csv" | head -1)
python3 tools/step_gaps.py "$F" > "$OUT/${TAG}_step_gaps.txt"
rm -rf "$OUT/_gt"
cat "$OUT/${TAG}_step_gaps.txt"
