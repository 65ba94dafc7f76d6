# usage: bash scripts/prof_tet_full.sh <out_dir>
# rocprofv3 kernel traces of the tet renderer at C3 (scripts/time_tet.py, 20 steps): one run with the default backward and
# one run of its own with full gradients (TetRenderer(full_grads=True): k_tet_backward_seq<float*, float*>), each under its
# own time limit -> <out_dir>/kernel_stats_tet_{default,full}.csv (+ the JSON line of each run)
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p "$1"
OUT=$(cd "$1" && pwd)
cd "$ROOT"
for mode in default full; do
    flag=""; [ $mode = full ] && flag=--full-grads
    timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/trace_$mode" -- \
        python3 scripts/time_tet.py --steps 20 $flag > "$OUT/tet_c3_$mode.json" 2> "$OUT/trace_$mode.err"
    cp "$OUT"/trace_$mode/*/*_kernel_stats.csv "$OUT/kernel_stats_tet_$mode.csv"
    grep -i "tet_backward\|tet_forward" "$OUT/kernel_stats_tet_$mode.csv" | cut -c1-200
done
