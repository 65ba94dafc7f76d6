# usage: bash scripts/prof_fragment_grads.sh <out_dir>
# rocprofv3 kernel trace of the tri renderer at C4 (scripts/time_tri.py, 20 steps) with fragments=4 and a gradient for every stored
# pair's barycentrics in the backward (k_tri_fragment_grads behind k_tri_backward_hits), at the reference's gradient level and with
# camera_grads, one run each, each under its own time limit; no counters.
# -> <out_dir>/kernel_stats_tri_fragment_grads_{default,camera}.csv (+ the JSON line of each run)
set -e -o pipefail
ROOT=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p "$1"
OUT=$(cd "$1" && pwd)
cd "$ROOT"
for grads in default camera; do
    timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/trace_tri_fragment_grads_$grads" -- \
        python3 scripts/time_tri.py --steps 20 --fragments 4 --fragment-grads --grads $grads > "$OUT/tri_fragment_grads_$grads.json" \
        2> "$OUT/trace_tri_fragment_grads_$grads.err"
    cp "$OUT"/trace_tri_fragment_grads_$grads/*/*_kernel_stats.csv "$OUT/kernel_stats_tri_fragment_grads_$grads.csv"
    grep -i "fragment_grads\|backward_hits\|tri_fragments\|backward_pix" "$OUT/kernel_stats_tri_fragment_grads_$grads.csv" | cut -c1-200
done
