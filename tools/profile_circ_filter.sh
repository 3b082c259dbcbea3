#!/bin/bash
# Device times of sei_circ_filter_sep and sei_blur_sep_circ from one rocprofv3 kernel trace (run on the GPU box from the
# repository root, library built):   tools/profile_circ_filter.sh OUTDIR
# Writes OUTDIR/q_kernel_trace.csv, OUTDIR/q_kernel_stats.csv and OUTDIR/circ_filter_times.csv (tools/exp_circ_filter.py).
R="$(cd "$(dirname "$0")/.." && pwd)"
OUT="${1:?output directory}"
mkdir -p "$OUT"
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT" -o q -- python3 "$R/tools/exp_circ_filter.py" > "$OUT/run.log" 2>&1 &&
    TRACE="$(find "$OUT" -name 'q_kernel_trace.csv' | head -1)" &&
    timeout 60 python3 "$R/tools/exp_circ_filter.py" --summarize "$TRACE" "$OUT/circ_filter_times.csv"
