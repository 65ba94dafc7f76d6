# usage: bash scripts/prof_mlp.sh <out_dir>
# The fused row MLP (fragments.mlp_rows_fused / RowMLP, scripts/time_mlp.py) in the packed deferred-shading chain, against
# nn.Sequential on the same Parameters: C4 with fragments=4, MLP C -> 64 -> 3 (tanh), C = 3 and C = 32:
#   * a rocprofv3 kernel trace of 23 steps (3 warm-up + 20), every step rendering the lists and running the chain with
#     nn.Sequential and with RowMLP forward + backward, so that the two new kernels stand next to the kernels torch launches for
#     the same MLP in the same run; no counters (a counter run is a run of its own);
#   * untraced: three alternating runs of each chain (wall time, peak memory), the MLP alone by events, dL_dW at the full N
#     against float64 torch.
# One run each, each under its own time limit; plain lines under set -e: the first step that fails ends the script, nothing is
# started after it.
# -> <out_dir>/kernel_stats_c{3,32}.csv, trace_c{3,32}.json, compare_c{3,32}.json
set -e -o pipefail
ROOT=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p "$1"
OUT=$(cd "$1" && pwd)
cd "$ROOT"
for C in 3 32; do
    timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/trace_c$C" -- \
        python3 scripts/time_mlp.py --steps 20 --channels $C > "$OUT/trace_c$C.json" 2> "$OUT/trace_c$C.err"
    cp "$OUT"/trace_c$C/*/*_kernel_stats.csv "$OUT/kernel_stats_c$C.csv"
    grep -i "k_mlp_\|Cijk\|gemm\|tanh\|elementwise\|reduce_kernel" "$OUT/kernel_stats_c$C.csv" | cut -c1-220
    timeout -k 10 400 python3 scripts/time_mlp.py --steps 20 --channels $C --compare > "$OUT/compare_c$C.json"
    cat "$OUT/compare_c$C.json"
done
