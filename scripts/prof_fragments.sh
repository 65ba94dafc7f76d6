# usage: bash scripts/prof_fragments.sh <out_dir>
# rocprofv3 kernel traces of the tri renderer at C4 (scripts/time_tri.py, 20 steps) without and with the fragment output
# (fragments=4: k_tri_fragments behind k_tri_forward<true, false>), one run each, each under its own time limit; no counters.
# -> <out_dir>/kernel_stats_tri_{default,fragments}.csv (+ the JSON line of each run)
set -e -o pipefail
ROOT=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p "$1"
OUT=$(cd "$1" && pwd)
cd "$ROOT"
for mode in default fragments; do
    flag=""; [ $mode = fragments ] && flag="--fragments 4"
    timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/trace_tri_$mode" -- \
        python3 scripts/time_tri.py --steps 20 $flag > "$OUT/tri_$mode.json" 2> "$OUT/trace_tri_$mode.err"
    cp "$OUT"/trace_tri_$mode/*/*_kernel_stats.csv "$OUT/kernel_stats_tri_$mode.csv"
    grep -i "tri_forward\|tri_fragments\|backward_pix" "$OUT/kernel_stats_tri_$mode.csv" | cut -c1-200
done
