# usage: bash scripts/prof_tet_fragments.sh <out_dir>
# rocprofv3 kernel traces of the tet renderer at C3 (scripts/time_tet.py, 20 steps) without and with the fragment output
# (fragments=8 and fragments=32: k_tet_fragments behind k_tet_forward), one run each, each under its own time limit; no counters.
# -> <out_dir>/kernel_stats_tet_{default,fragments8,fragments32}.csv (+ the JSON line of each run)
set -e -o pipefail
ROOT=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p "$1"
OUT=$(cd "$1" && pwd)
cd "$ROOT"
for mode in default fragments8 fragments32; do
    flag=""; [ $mode != default ] && flag="--fragments ${mode#fragments}"
    timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/trace_tet_$mode" -- \
        python3 scripts/time_tet.py --steps 20 $flag > "$OUT/tet_$mode.json" 2> "$OUT/trace_tet_$mode.err"
    cp "$OUT"/trace_tet_$mode/*/*_kernel_stats.csv "$OUT/kernel_stats_tet_$mode.csv"
    grep -i "tet_forward\|tet_fragments\|tet_backward" "$OUT/kernel_stats_tet_$mode.csv" | cut -c1-200
done
