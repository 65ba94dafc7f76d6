# usage: bash scripts/prof_texture.sh <out_dir>
# fragments.composite_texture_fused at C4 with fragments=4, a 1024 x 1024 x 3 texture, planar UVs, gradients to opacity, texture
# and UVs (scripts/time_texture.py):
#   * a rocprofv3 kernel trace of 23 steps (3 warm-up + 20), every step rendering the lists (k_tri_fragments) and running
#     k_composite_fragments + _backward (C = 3: the yardstick) and k_composite_texture + _backward over them; no counters;
#   * untraced, wall time and peak memory of one forward + backward against fragments.composite_texture (plain torch) on the
#     same lists, and the distinct texels per tile against the backward's table.
# One run each, each under its own time limit.
# -> <out_dir>/kernel_stats.csv, <out_dir>/trace.json, <out_dir>/compare.json
set -e -o pipefail
ROOT=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p "$1"
OUT=$(cd "$1" && pwd)
cd "$ROOT"
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/trace" -- \
    python3 scripts/time_texture.py --steps 20 > "$OUT/trace.json" 2> "$OUT/trace.err"
cp "$OUT"/trace/*/*_kernel_stats.csv "$OUT/kernel_stats.csv"
grep -i "composite_\|tri_fragments" "$OUT/kernel_stats.csv" | cut -c1-220
timeout -k 10 300 python3 scripts/time_texture.py --steps 8 --compare > "$OUT/compare.json"
cat "$OUT/compare.json"
