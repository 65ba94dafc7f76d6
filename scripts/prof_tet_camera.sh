# usage: bash scripts/prof_tet_camera.sh <out_dir>
# rocprofv3 kernel traces of the tet renderer at C3 (scripts/time_tet.py, 20 steps), one run per backward variant, each
# under its own time limit: the default gradients (k_tet_backward_seq<>), full_grads=True (<float*, float*>) and
# camera_grads=True (<float*, float*, float*> + k_tri_camera_reduce<64>) -> <out_dir>/kernel_stats_tet_{default,full,camera}.csv
# (+ the JSON line of each run).  VGPRs / LDS per workgroup: the kernel trace CSVs (arch_vgpr_count, lds_block_size).
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p "$1"
OUT=$(cd "$1" && pwd)
cd "$ROOT"
for mode in default full camera; do
    flag=""; [ $mode = full ] && flag=--full-grads; [ $mode = camera ] && flag=--camera-grads
    timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/trace_$mode" -- \
        python3 scripts/time_tet.py --steps 20 $flag > "$OUT/tet_c3_$mode.json" 2> "$OUT/trace_$mode.err"
    cp "$OUT"/trace_$mode/*/*_kernel_stats.csv "$OUT/kernel_stats_tet_$mode.csv"
    cp "$OUT"/trace_$mode/*/*_kernel_trace.csv "$OUT/kernel_trace_tet_$mode.csv"
    grep -i "tet_backward\|camera_reduce" "$OUT/kernel_stats_tet_$mode.csv" | cut -c1-200
done
