#!/bin/bash
# The roofline kernel two ways on one box: bench.py's in-run HIP-event timing of the
# 128->128 @128^2 B=64 Winograd conv, and the rocprofv3 kernel-trace summary of the same
# kernel / shape launched 20 times (tools/prof_conv.py).
#   tools/gpu_roofline_prof.sh OUT_DIR
O=${1:?usage: tools/gpu_roofline_prof.sh OUT_DIR}; mkdir -p "$O"; export TMPDIR=/tmp
timeout -k 10 300 python bench.py --full --steps 5 --no-train --no-pinn --no-dps --no-cpu-baseline > "$O/roof_bench.json" 2> "$O/roof_bench.err" || { tail -5 "$O/roof_bench.err"; exit 1; }
python -c "import json,sys;d=json.load(open(sys.argv[1]));print('bench roofline ms/launch', d['roofline']['ms_per_launch'])" "$O/roof_bench.json"
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d "$O/prof_roof" -o roof --output-format csv -- python tools/prof_conv.py > "$O/prof_roof.log" 2>&1 || { tail -5 "$O/prof_roof.log"; exit 1; }
python - "$O/prof_roof/roof_kernel_stats.csv" <<'PY'
import csv
import sys
for r in csv.DictReader(open(sys.argv[1])):
    if "wino_f23" in r["Name"]:
        print("rocprof", r["Name"][:60], r["Calls"], "avg ms", float(r["AverageNs"]) / 1e6)
PY
