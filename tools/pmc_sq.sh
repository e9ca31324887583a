#!/bin/bash
# SQ-level counters of the headline kernels (issue / stall split, effective clock): development aid
#   usage: bash tools/pmc_sq.sh [OUT_DIR, default out/pmc_sq]
set -o pipefail
R="$(cd "$(dirname "$0")/.." && pwd)"; OUT="$(realpath -m "${1:-$R/out/pmc_sq}")"; rm -rf "$OUT"; mkdir -p "$OUT"; export TMPDIR=/tmp; cd /tmp
timeout -k 10 500 rocprofv3 --pmc SQ_WAVE_CYCLES SQ_WAIT_INST_ANY SQ_WAIT_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_INSTS_VALU GRBM_GUI_ACTIVE --kernel-trace --output-format csv -d "$OUT" -- \
  python3 "$R/bench.py" --full --steps 2 --warmup 1 --no-cpu-baseline --replay none --no-extras --no-live-pmc > "$OUT/out.json" 2> "$OUT/err.txt" || { tail -5 "$OUT/err.txt"; exit 1; }
OUT="$OUT" python3 - <<'PY'
import csv, glob, os
from collections import defaultdict
acc = defaultdict(lambda: defaultdict(lambda: [0.0, 0]))
for f in glob.glob(os.path.join(os.environ['OUT'], '**', '*counter_collection.csv'), recursive=True):
    for r in csv.DictReader(open(f)):
        n = r['Kernel_Name'].split('(')[0].replace('void ', '')
        if n == 'hm::msm_accumulate_kernel' or n.startswith('hm::ntt_pass_kernel<11'):
            a = acc[n][r['Counter_Name']]; a[0] += float(r['Counter_Value']); a[1] += 1
for n, d in acc.items():
    print(n, {k: round(v[0] / v[1]) for k, v in d.items()})
PY
