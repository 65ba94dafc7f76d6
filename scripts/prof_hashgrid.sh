# usage: bash scripts/prof_hashgrid.sh <out_dir>
# The fused hash-grid encoding (fragments.hashgrid_rows_fused / HashGrid, scripts/time_hashgrid.py) in front of the fused row MLP,
# on the hit points of C4 with fragments=4: 16 levels x 2 features, T = 2^19, R = 16 .. 2006, then RowMLP(32, 64, 3):
#   * a rocprofv3 kernel trace of 23 steps (3 warm-up + 20), every step rendering the lists and running HashGrid -> RowMLP forward
#     + backward, so that the new kernels stand next to k_mlp_rows and k_mlp_rows_backward of the same run; no counters (a
#     counter run is a run of its own);
#   * untraced: the new kernels alone by events, on the lists' row order and on the rows shuffled (product library);
#   * the same on the ablation build, once per switch: as built, the forward's (row block, level chunk) grid, its per-lane row
#     stores, the backward without the LDS table, its direct atomics one lane per row (16777216), and the first and the table-less one
#     again with the counters on (8388608: the per-level share of
#     dL/dtable contributions that left as direct atomics; the counters cost time, so those runs' times mean nothing);
#   * untraced: three alternating runs against the torch models on the device (wall time, peak memory), dL_dtable at the full N
#     against float64 torch.
# One run each, each under its own time limit; plain lines under set -e: the first step that fails ends the script, nothing is
# started after it.
# -> <out_dir>/kernel_stats.csv, trace.json, kernels.json, kernels_ablation_{0,1048576,2097152,4194304,16777216,8388608,12582912}.json, compare.json
set -e -o pipefail
ROOT=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p "$1"
OUT=$(cd "$1" && pwd)
cd "$ROOT"
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/trace" -- \
    python3 scripts/time_hashgrid.py --steps 20 > "$OUT/trace.json" 2> "$OUT/trace.err"
cp "$OUT"/trace/*/*_kernel_stats.csv "$OUT/kernel_stats.csv"
grep -i "k_hashgrid_\|k_mlp_" "$OUT/kernel_stats.csv" | cut -c1-220
timeout -k 10 200 python3 scripts/time_hashgrid.py --steps 20 --kernels > "$OUT/kernels.json"
cat "$OUT/kernels.json"
ABL="$ROOT/dmesh_renderer_amd/libdmesh_renderer_hip_ablation.so"
for BITS in 0 1048576 2097152 4194304 16777216 8388608 12582912; do
    DMR_LIBRARY="$ABL" DMR_ABLATE=$BITS timeout -k 10 200 python3 scripts/time_hashgrid.py --steps 20 --kernels > "$OUT/kernels_ablation_$BITS.json"
    cat "$OUT/kernels_ablation_$BITS.json"
done
timeout -k 10 500 python3 scripts/time_hashgrid.py --steps 20 --compare > "$OUT/compare.json"
cat "$OUT/compare.json"
