# usage: bash scripts/prof_sh.sh <out_dir>
# The fused view-direction encoding (fragments.sh_rows_fused / ViewSH, scripts/time_sh.py) beside the fused hash grid in front of
# the fused row MLP, on the hit points of C4 with fragments=4: cat(HashGrid 16 x 2, ViewSH(4)) -> RowMLP(48, 64, 3):
#   * a rocprofv3 kernel trace of 23 steps (3 warm-up + 20), every step rendering the lists and running the chain forward +
#     backward, so that the new kernels stand next to k_hashgrid_rows and k_mlp_rows of the same run; no counters (a counter run
#     is a run of its own);
#   * untraced: the new kernels alone by events, per degree (product library);
#   * the same on the ablation build, as built and with every degree's other store / load shape (33554432): the store-shape table;
#   * untraced: three alternating runs against the torch model on the device and of the chain with and without the direction
#     (wall time, peak memory), the th.cat's cost, dL_dorigin at the full N against float64 torch.
# One run each, each under its own time limit; plain lines under set -e: the first step that fails ends the script, nothing is
# started after it.
# -> <out_dir>/kernel_stats.csv, trace.json, kernels.json, kernels_ablation_{0,33554432}.json, compare.json
set -e -o pipefail
ROOT=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p "$1"
OUT=$(cd "$1" && pwd)
cd "$ROOT"
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/trace" -- \
    python3 scripts/time_sh.py --steps 20 > "$OUT/trace.json" 2> "$OUT/trace.err"
cp "$OUT"/trace/*/*_kernel_stats.csv "$OUT/kernel_stats.csv"
grep -i "k_sh_\|k_hashgrid_\|k_mlp_\|k_interpolate_packed" "$OUT/kernel_stats.csv" | cut -c1-220
timeout -k 10 200 python3 scripts/time_sh.py --steps 20 --kernels > "$OUT/kernels.json"
cat "$OUT/kernels.json"
ABL="$ROOT/dmesh_renderer_amd/libdmesh_renderer_hip_ablation.so"
for BITS in 0 33554432; do
    DMR_LIBRARY="$ABL" DMR_ABLATE=$BITS timeout -k 10 200 python3 scripts/time_sh.py --steps 20 --kernels > "$OUT/kernels_ablation_$BITS.json"
    cat "$OUT/kernels_ablation_$BITS.json"
done
timeout -k 10 500 python3 scripts/time_sh.py --steps 20 --compare > "$OUT/compare.json"
cat "$OUT/compare.json"
