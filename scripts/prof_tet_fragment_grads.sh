# usage: bash scripts/prof_tet_fragment_grads.sh <out_dir>
# rocprofv3 kernel trace of the tet renderer at C3 (scripts/time_tet.py, 20 steps) with fragments=8 and a gradient for every stored
# pair's barycentrics in the backward (k_tet_fragment_grads behind k_tet_backward_seq), at the level the option implies
# (full_grads) and with camera_grads, one run each, each under its own time limit; no counters.
# -> <out_dir>/kernel_stats_tet_fragment_grads_{default,camera}.csv (+ the JSON line of each run)
set -e -o pipefail
ROOT=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p "$1"
OUT=$(cd "$1" && pwd)
cd "$ROOT"
for grads in default camera; do
    flag=""; [ $grads = camera ] && flag="--camera-grads"
    timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/trace_tet_fragment_grads_$grads" -- \
        python3 scripts/time_tet.py --steps 20 --fragments 8 --fragment-grads $flag > "$OUT/tet_fragment_grads_$grads.json" \
        2> "$OUT/trace_tet_fragment_grads_$grads.err"
    cp "$OUT"/trace_tet_fragment_grads_$grads/*/*_kernel_stats.csv "$OUT/kernel_stats_tet_fragment_grads_$grads.csv"
    grep -i "fragment_grads\|tet_backward\|tet_fragments\|tet_forward" "$OUT/kernel_stats_tet_fragment_grads_$grads.csv" | cut -c1-200
done
