# usage: bash scripts/prof_composite_fused.sh <out_dir>
# fragments.composite_fused at C4 with fragments=4 (scripts/time_composite_fused.py), C = 3 and C = 32 channels:
#   * a rocprofv3 kernel trace of 23 steps each (3 warm-up + 20), every step rendering the lists (k_tri_fragments) and running
#     k_composite_fragments + k_composite_fragments_backward over them; no counters;
#   * untraced, wall time and peak memory of one forward + backward against fragments.composite (plain torch) on the same lists.
# One run each, each under its own time limit.
# -> <out_dir>/kernel_stats_c{3,32}.csv, <out_dir>/trace_c{3,32}.json, <out_dir>/compare_c{3,32}.json
set -e -o pipefail
ROOT=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p "$1"
OUT=$(cd "$1" && pwd)
cd "$ROOT"
for c in 3 32; do
    timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/trace_c$c" -- \
        python3 scripts/time_composite_fused.py --steps 20 --channels $c > "$OUT/trace_c$c.json" 2> "$OUT/trace_c$c.err"
    cp "$OUT"/trace_c$c/*/*_kernel_stats.csv "$OUT/kernel_stats_c$c.csv"
    grep -i "composite_fragments\|tri_fragments\|tri_forward" "$OUT/kernel_stats_c$c.csv" | cut -c1-220
    timeout -k 10 300 python3 scripts/time_composite_fused.py --steps 20 --channels $c --compare > "$OUT/compare_c$c.json"
    cat "$OUT/compare_c$c.json"
done
