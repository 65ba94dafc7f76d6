# usage: bash scripts/prof_envmap_lod.sh <out_dir>
# The fused pyramid lookup (fragments.envmap_pyramid_fused / envmap_lod_rows_fused / EnvMapPyramid, scripts/time_envmap_lod.py) on C4
# with fragments=4, C = 3, on the background's rows (N = B H W) and the packed rows, as they are and shuffled, lod uniform over
# [0, L-1]:
#   * a rocprofv3 kernel trace of 23 steps (3 warm-up + 20), every step one forward + backward of EnvMapPyramid(256, 512) and of
#     EnvMap(256, 512) on both row sets, so that the new kernels stand next to k_envmap_rows and k_envmap_rows_backward of the same
#     run; no counters (a counter run is a run of its own);
#   * untraced: the new kernels alone by events, both pyramid sizes with the full L, the four row sets, each gradient alone, the
#     single-level pair on the same rows, and the builder next to the torch builder;
#   * on the ablation build (python -m dmesh_renderer_amd.build --ablation) with the counters of dL/dpyramid's direct atomics
#     (268435456): their share per pyramid size and row set;
#   * untraced: three alternating runs against the torch models on the device (wall time, peak memory) and the deviation of y and the
#     three gradients from float64 torch on the device.
# One run each, each under its own time limit; plain lines under set -e: the first step that fails ends the script, nothing is
# started after it.
# -> <out_dir>/kernel_stats.csv, trace.json, kernels.json, atomics_ablation_268435456.json, compare.json
set -e -o pipefail
ROOT=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p "$1"
OUT=$(cd "$1" && pwd)
cd "$ROOT"
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/trace" -- \
    python3 scripts/time_envmap_lod.py --steps 20 > "$OUT/trace.json" 2> "$OUT/trace.err"
cp "$OUT"/trace/*/*_kernel_stats.csv "$OUT/kernel_stats.csv"
grep -i "k_envmap_\|k_rows_fill" "$OUT/kernel_stats.csv" | cut -c1-220
timeout -k 10 300 python3 scripts/time_envmap_lod.py --steps 20 --kernels > "$OUT/kernels.json"
cat "$OUT/kernels.json"
ABL="$ROOT/dmesh_renderer_amd/libdmesh_renderer_hip_ablation.so"
DMR_LIBRARY="$ABL" DMR_ABLATE=268435456 timeout -k 10 200 python3 scripts/time_envmap_lod.py --stats > "$OUT/atomics_ablation_268435456.json"
cat "$OUT/atomics_ablation_268435456.json"
timeout -k 10 500 python3 scripts/time_envmap_lod.py --steps 20 --compare > "$OUT/compare.json"
cat "$OUT/compare.json"
