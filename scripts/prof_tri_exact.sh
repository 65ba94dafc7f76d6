# usage: bash scripts/prof_tri_exact.sh <out_dir>
# rocprofv3 kernel traces of the tri renderer at C4 (scripts/time_tri.py, 20 steps), one run per backward variant, each
# under its own time limit: the reference's gradients (k_tri_backward_hits<0>), exact_grads=True (<1>) and
# camera_grads=True (<2, float*> + k_tri_camera_reduce) -> <out_dir>/kernel_stats_tri_{default,exact,camera}.csv
# (+ the JSON line of each run).  VGPRs / LDS per workgroup: the kernel trace CSVs (arch_vgpr_count, lds_block_size).
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p "$1"
OUT=$(cd "$1" && pwd)
cd "$ROOT"
for mode in default exact camera; do
    timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/trace_$mode" -- \
        python3 scripts/time_tri.py --steps 20 --grads $mode > "$OUT/tri_c4_$mode.json" 2> "$OUT/trace_$mode.err"
    cp "$OUT"/trace_$mode/*/*_kernel_stats.csv "$OUT/kernel_stats_tri_$mode.csv"
    cp "$OUT"/trace_$mode/*/*_kernel_trace.csv "$OUT/kernel_trace_tri_$mode.csv"
    grep -i "backward_hits\|camera_reduce" "$OUT/kernel_stats_tri_$mode.csv" | cut -c1-200
done
