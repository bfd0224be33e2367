#!/bin/bash
# rocprofv3 kernel-trace statistics of one bench workload -> $OUT/<tag>_kernel_stats.csv (OUT: profile_out)
# Usage: bash tools/kernel_stats.sh <workload> <tag> [extra bench args]
set -e
WL=$1; TAG=$2; shift 2
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
OUT=${OUT:-profile_out}; mkdir -p "$OUT"
rm -rf "$OUT/_kt"
rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/_kt" -o k -- python3 bench.py --full --workload $WL --steps 50 --warmup 5 --no-cpu-baseline --no-other-workloads "$@" > "$OUT/${TAG}_kt.json" 2> "$OUT/${TAG}_kt.err"
find "$OUT/_kt" -name "*kernel_stats.csv" -exec cp {} "$OUT/${TAG}_kernel_stats.csv" \;
rm -rf "$OUT/_kt"
python3 - <<PY
import csv
rows = list(csv.DictReader(open("$OUT/${TAG}_kernel_stats.csv")))
for r in rows[:16]:
    print(f"{r['Name'][:64]:64s} calls {r['Calls']:>5s} avg_us {float(r['AverageNs'])/1e3:9.1f} pct {r['Percentage']}")
PY
