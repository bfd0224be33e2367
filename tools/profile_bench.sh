#!/bin/bash
# rocprofv3 evidence for one bench workload (run on the GPU box): kernel-trace statistics, HBM bytes (FETCH_SIZE / WRITE_SIZE
# in separate counter passes) and MFMA-pipe utilisation, all of `python3 bench.py --full --workload <wl> ...`.
#   bash tools/profile_bench.sh <workload> <tag> [mlp kernel-name substrings for the time-weighted MFMA figure ...]
# -> $OUT/<tag>_kernel_stats.csv, <tag>_bench_under_rocprof.json, <tag>_pmc_summary.json, <tag>_mfma_util.json (OUT: profile_out)
set -e
WL=$1; TAG=$2; shift 2
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
OUT=${OUT:-profile_out}; mkdir -p "$OUT"
rm -rf "$OUT/_kt" "$OUT/_pf" "$OUT/_pw" "$OUT/_pm"
rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/_kt" -o k -- python3 bench.py --full --workload $WL --steps 50 --warmup 5 --no-cpu-baseline --no-other-workloads > "$OUT/${TAG}_bench_under_rocprof.json" 2> "$OUT/${TAG}_kt.err"
find "$OUT/_kt" -name "*kernel_stats.csv" -exec cp {} "$OUT/${TAG}_kernel_stats.csv" \;
echo "kernel trace done"
ARGS="bench.py --full --workload $WL --steps 3 --warmup 1 --no-cpu-baseline --no-other-workloads --no-kernel-timers"
rocprofv3 --pmc FETCH_SIZE --output-format csv -d "$OUT/_pf" -o f -- python3 $ARGS > /dev/null 2> "$OUT/${TAG}_fetch.err"
echo "fetch pass done"
rocprofv3 --pmc WRITE_SIZE --output-format csv -d "$OUT/_pw" -o w -- python3 $ARGS > /dev/null 2> "$OUT/${TAG}_write.err"
echo "write pass done"
rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE SQ_ACTIVE_INST_VALU SQ_WAVE_CYCLES SQ_WAIT_INST_ANY --output-format csv -d "$OUT/_pm" -o m -- python3 $ARGS > /dev/null 2> "$OUT/${TAG}_mfma.err"
echo "mfma pass done"
F=$(find "$OUT/_pf" -name "*counter_collection.csv" | head -1)
W=$(find "$OUT/_pw" -name "*counter_collection.csv" | head -1)
M=$(find "$OUT/_pm" -name "*counter_collection.csv" | head -1)
python3 profiles/pmc_summary_generic.py "$F" "$W" 4 "$OUT/${TAG}_pmc_summary.json"
python3 profiles/mfma_util_generic.py "$M" "$OUT/${TAG}_mfma_util.json" "$@" | tail -12
rm -rf "$OUT/_kt" "$OUT/_pf" "$OUT/_pw" "$OUT/_pm"
head -14 "$OUT/${TAG}_kernel_stats.csv" | cut -c1-200
