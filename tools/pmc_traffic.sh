#!/bin/bash
# HBM traffic of the dominant kernels from the PMC counters, as MI355X_MICROARCH.md §HBM prescribes:
# FETCH_SIZE and WRITE_SIZE in SEPARATE rocprofv3 passes (TCC slots), counters in their own runs
# (no sys/hip/hsa trace domains), program directly after `--`.
#   usage: bash tools/pmc_traffic.sh [OUT_DIR, default out/pmc]
set -o pipefail
R="$(cd "$(dirname "$0")/.." && pwd)"; OUT="$(realpath -m "${1:-$R/out/pmc}")"
rm -rf "$OUT"; mkdir -p "$OUT"     # a fresh directory: the summary averages every CSV it finds
export TMPDIR=/tmp
cd /tmp
for ctr in FETCH_SIZE WRITE_SIZE; do
  timeout -k 10 500 rocprofv3 --pmc $ctr --kernel-trace --output-format csv -d "$OUT/$ctr" -- \
    python3 "$R/bench.py" --full --steps 2 --warmup 1 --no-cpu-baseline --replay none --no-extras --no-live-pmc > "$OUT/$ctr.json" 2> "$OUT/$ctr.err" || { tail -5 "$OUT/$ctr.err"; exit 1; }
done
python3 "$R/tools/pmc_summarise.py" "$OUT" > "$OUT/summary.json" && cat "$OUT/summary.json"
