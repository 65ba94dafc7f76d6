# usage: bash scripts/prof_packed.sh <out_dir>
# The packed deferred-shading path (fragments.pack_slots_fused + interpolate_packed_fused + composite_values_packed_fused,
# scripts/time_packed.py) against the dense fused path on the same lists:
#   * the fill fraction n_used / (B K H W) of the lists: C4 / fragments=4 (tri), C3 / fragments=8 and 32 (tet);
#   * at C4 / fragments=4, C = 3 and C = 32: a rocprofv3 kernel trace of 23 steps (3 warm-up + 20), every step rendering the
#     lists and running the dense chain and the packed chain forward + backward, so that every new kernel stands next to its
#     dense counterpart in the same run; no counters;
#   * untraced: one forward + backward with a two-layer MLP (C -> 64 -> 3, tanh) between the ends, packed against dense (the dense
#     path with the permutes a linear layer needs): wall time, peak memory, each kernel's device time, the pack launches alone.
# One run each, each under its own time limit; plain lines under set -e: the first step that fails ends the script, nothing is
# started after it.
# -> <out_dir>/fill_fractions.jsonl, kernel_stats_c{3,32}.csv, trace_c{3,32}.json, compare_c{3,32}.json
set -e -o pipefail
ROOT=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p "$1"
OUT=$(cd "$1" && pwd)
cd "$ROOT"
timeout -k 10 200 python3 scripts/time_packed.py --fill --config C4 --fragments 4 > "$OUT/fill_fractions.jsonl"
timeout -k 10 200 python3 scripts/time_packed.py --fill --config C3 --fragments 8 >> "$OUT/fill_fractions.jsonl"
timeout -k 10 200 python3 scripts/time_packed.py --fill --config C3 --fragments 32 >> "$OUT/fill_fractions.jsonl"
cat "$OUT/fill_fractions.jsonl"
for C in 3 32; do
    timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/trace_c$C" -- \
        python3 scripts/time_packed.py --steps 20 --channels $C > "$OUT/trace_c$C.json" 2> "$OUT/trace_c$C.err"
    cp "$OUT"/trace_c$C/*/*_kernel_stats.csv "$OUT/kernel_stats_c$C.csv"
    grep -i "packed\|k_pack_\|interpolate_fragments\|composite_values\|tri_fragments\|deferred_zero" "$OUT/kernel_stats_c$C.csv" | cut -c1-220
    timeout -k 10 400 python3 scripts/time_packed.py --steps 20 --channels $C --compare > "$OUT/compare_c$C.json"
    cat "$OUT/compare_c$C.json"
done
# The two store shapes of k_interpolate_packed (profiles/packed/store_shapes.txt): the ablation build (python -m dmesh_renderer_amd.build
# --ablation), DMR_ABLATE=0 (the shape the product uses at that C) against 32768 (the other one), fresh processes alternating.
ABL="$ROOT/dmesh_renderer_amd/libdmesh_renderer_hip_ablation.so"
if [ -f "$ABL" ]; then
    : > "$OUT/store_shapes.jsonl"
    for C in 3 4 5 8 16 24 32; do
        for A in 0 32768 0 32768; do
            DMR_LIBRARY="$ABL" DMR_ABLATE=$A timeout -k 10 200 python3 scripts/time_packed.py --forward-only --steps 20 --channels $C >> "$OUT/store_shapes.jsonl"
        done
    done
    cut -c1-60,200-600 "$OUT/store_shapes.jsonl"
fi
