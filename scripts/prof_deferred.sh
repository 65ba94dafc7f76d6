# usage: bash scripts/prof_deferred.sh <out_dir>
# fragments.interpolate_fused + composite_values_fused at C4 with fragments=4, all gradients (scripts/time_deferred.py), at C = 3 and C = 32:
#   * a rocprofv3 kernel trace of 23 steps (3 warm-up + 20), every step rendering the lists (k_tri_fragments), compositing the same
#     attributes with composite_fused (k_composite_fragments, k_composite_fragments_backward) and running the four new kernels;
#     no counters;
#   * untraced, wall time and peak memory of one forward + backward against fragments.interpolate + composite_values (plain
#     torch) on the same lists, and each new kernel's device time.
# One run each, each under its own time limit; plain lines under set -e: the first step that fails ends the script, nothing is
# started after it.
# -> <out_dir>/kernel_stats_c{3,32}.csv, <out_dir>/trace_c{3,32}.json, <out_dir>/compare_c{3,32}.json
set -e -o pipefail
ROOT=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p "$1"
OUT=$(cd "$1" && pwd)
cd "$ROOT"
for C in 3 32; do
    timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/trace_c$C" -- \
        python3 scripts/time_deferred.py --steps 20 --channels $C > "$OUT/trace_c$C.json" 2> "$OUT/trace_c$C.err"
    cp "$OUT"/trace_c$C/*/*_kernel_stats.csv "$OUT/kernel_stats_c$C.csv"
    grep -i "interpolate_fragments\|composite_values\|composite_fragments\|tri_fragments\|deferred_zero" "$OUT/kernel_stats_c$C.csv" | cut -c1-220
    timeout -k 10 400 python3 scripts/time_deferred.py --steps 20 --channels $C --compare > "$OUT/compare_c$C.json"
    cat "$OUT/compare_c$C.json"
done
