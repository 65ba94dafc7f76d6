# usage: bash scripts/prof_surface.sh <out_dir>
# The fused surface frame (fragments.surface_packed_fused, scripts/time_surface.py) on C4 with fragments=4:
#   * a rocprofv3 kernel trace of 23 steps (3 warm-up + 20), every step one forward + backward of surface_packed_fused and of
#     interpolate_packed_fused(verts) at C = 3 on the same lists, so that the new kernels stand next to k_interpolate_packed and
#     k_interpolate_packed_backward of the same run; no counters (a counter run is a run of its own);
#   * untraced: the new kernels by events -- the forward, the backward for all three gradients and for each alone -- with the
#     bytes moved by construction per second;
#   * untraced: three alternating runs against the torch model on the device (wall time, peak memory) and dL_dverts, dL_dbary,
#     dL_dorigin at the workload's own N against float64 torch on the device.
# One run each, each under its own time limit; plain lines under set -e: the first step that fails ends the script, nothing is
# started after it.
# -> <out_dir>/kernel_stats.csv, trace.json, kernels.json, compare.json
set -e -o pipefail
ROOT=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p "$1"
OUT=$(cd "$1" && pwd)
cd "$ROOT"
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/trace" -- \
    python3 scripts/time_surface.py --steps 20 > "$OUT/trace.json" 2> "$OUT/trace.err"
cp "$OUT"/trace/*/*_kernel_stats.csv "$OUT/kernel_stats.csv"
grep -i "k_surface_\|k_interpolate_packed\|k_rows_fill\|k_deferred_zero" "$OUT/kernel_stats.csv" | cut -c1-220
timeout -k 10 200 python3 scripts/time_surface.py --steps 20 --kernels > "$OUT/kernels.json"
cat "$OUT/kernels.json"
timeout -k 10 400 python3 scripts/time_surface.py --steps 20 --compare > "$OUT/compare.json"
cat "$OUT/compare.json"
