# usage: bash scripts/prof_visibility.sh <out_dir>
# fragments.face_visibility_fused at C4 with fragments=4, coverage=True, a pixel_weight, both gradients (scripts/time_visibility.py):
#   * a rocprofv3 kernel trace of 23 steps (3 warm-up + 20), every step rendering the lists (k_tri_fragments), compositing
#     verts_color over them (k_composite_fragments, C = 3) and running k_face_visibility + k_face_visibility_backward; no counters;
#   * untraced, wall time and peak memory of one forward + backward against fragments.face_visibility + face_coverage (plain
#     torch) on the same lists.
# One run each, each under its own time limit.
# -> <out_dir>/kernel_stats.csv, <out_dir>/trace.json, <out_dir>/compare.json
set -e -o pipefail
ROOT=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p "$1"
OUT=$(cd "$1" && pwd)
cd "$ROOT"
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/trace" -- \
    python3 scripts/time_visibility.py --steps 20 > "$OUT/trace.json" 2> "$OUT/trace.err" &&
cp "$OUT"/trace/*/*_kernel_stats.csv "$OUT/kernel_stats.csv" &&
grep -i "face_visibility\|composite_fragments\|tri_fragments" "$OUT/kernel_stats.csv" | cut -c1-220 &&
timeout -k 10 300 python3 scripts/time_visibility.py --steps 20 --compare > "$OUT/compare.json" &&
cat "$OUT/compare.json"
