# usage: bash scripts/prof_alpha.sh <out_dir>
# rocprofv3 kernel traces of both renderers with and without the alpha output, one run each, each under its own time
# limit: the tri renderer at C4 (scripts/time_tri.py, 20 steps: k_tri_forward<true, false> / <true, true>,
# k_tri_backward_pix<false, false> / <false, true>) and the tet renderer at C3 (scripts/time_tet.py, 20 steps:
# k_tet_forward<false> / <true>, k_tet_backward_seq<false> / <true>)
# -> <out_dir>/kernel_stats_{tri,tet}_{default,alpha}.csv (+ the JSON line of each run)
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p "$1"
OUT=$(cd "$1" && pwd)
cd "$ROOT"
for kind in tri tet; do
    for mode in default alpha; do
        flag=""; [ $mode = alpha ] && flag=--alpha
        timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/trace_${kind}_$mode" -- \
            python3 scripts/time_$kind.py --steps 20 $flag > "$OUT/${kind}_$mode.json" 2> "$OUT/trace_${kind}_$mode.err"
        cp "$OUT"/trace_${kind}_$mode/*/*_kernel_stats.csv "$OUT/kernel_stats_${kind}_$mode.csv"
        grep -i "tri_forward\|backward_pix\|tet_forward\|tet_backward" "$OUT/kernel_stats_${kind}_$mode.csv" | cut -c1-200
    done
done
