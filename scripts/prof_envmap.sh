# usage: bash scripts/prof_envmap.sh <out_dir>
# The fused environment-map lookup (fragments.envmap_rows_fused / EnvMap, scripts/time_envmap.py) on C4 with fragments=4, C = 3, on
# the background's rows (N = B H W) and the packed rows, as they are and shuffled:
#   * a rocprofv3 kernel trace of 23 steps (3 warm-up + 20), every step one forward + backward of EnvMap(256, 512) on both row
#     sets and of ViewSH(4) on the packed rows, so that the new kernels stand next to k_sh_rows and k_sh_rows_backward of the same
#     run; no counters (a counter run is a run of its own);
#   * untraced: the new kernels alone by events, both map sizes, the four row sets, the forward per C (product library);
#   * the same on the ablation build with the counters of dL/denvmap's direct atomics (134217728), as built and with every chunk
#     count's other store shape (+ 67108864): the store-shape table and the atomics' shares;
#   * untraced: three alternating runs against the torch model on the device (wall time, peak memory) and the float32 deviation
#     on large maps against float64 torch.
# One run each, each under its own time limit; plain lines under set -e: the first step that fails ends the script, nothing is
# started after it.
# -> <out_dir>/kernel_stats.csv, trace.json, kernels.json, kernels_ablation_{134217728,201326592}.json, compare.json
set -e -o pipefail
ROOT=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p "$1"
OUT=$(cd "$1" && pwd)
cd "$ROOT"
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/trace" -- \
    python3 scripts/time_envmap.py --steps 20 > "$OUT/trace.json" 2> "$OUT/trace.err"
cp "$OUT"/trace/*/*_kernel_stats.csv "$OUT/kernel_stats.csv"
grep -i "k_envmap_\|k_sh_rows\|k_rows_fill" "$OUT/kernel_stats.csv" | cut -c1-220
timeout -k 10 200 python3 scripts/time_envmap.py --steps 20 --kernels > "$OUT/kernels.json"
cat "$OUT/kernels.json"
ABL="$ROOT/dmesh_renderer_amd/libdmesh_renderer_hip_ablation.so"
for BITS in 134217728 201326592; do
    DMR_LIBRARY="$ABL" DMR_ABLATE=$BITS timeout -k 10 200 python3 scripts/time_envmap.py --steps 20 --kernels > "$OUT/kernels_ablation_$BITS.json"
    cat "$OUT/kernels_ablation_$BITS.json"
done
timeout -k 10 500 python3 scripts/time_envmap.py --steps 20 --compare > "$OUT/compare.json"
cat "$OUT/compare.json"
