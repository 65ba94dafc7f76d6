"""The scene pairs of tests/tri_placed_cases.py reach what they are for -- asserted on the CPU oracle alone, with bin_emit's
routes, k_build_placement's segments and the sort's rule restated by tri_placed_cases.classify -- and the constants that
restatement rests on are still in the sources as text.  Whether a pair fits its segments or leaves them is a condition on the
oracle's counts, stated here; nothing of it is tuned on the GPU.  tests/test_tri_placed_paths_gpu.py runs the pairs."""
import glob
import os
import re

import numpy as np
import pytest
import torch as th

import tri_placed_cases as PC

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "dmesh_renderer_amd", "csrc")

# The lines tri_placed_cases restates, each once in its file.
RESTATED = {
    "dmr_kernels.hpp": [
        "constexpr uint32_t SEG_SLACK = 32;",
        "constexpr int SCAN_SINGLE_MAX = 8192;",
        "constexpr int MASK_CHUNK = 128;",
        "return e > tile_offset[tile + 1] ? tile_offset[tile] : e;",
    ],
    "dmr_binning.hip": [
        "constexpr int LDS_HIST_MAX = 8192;",
        "constexpr uint32_t BIG_RECT = 256;",
        "constexpr int BIG_MAX = 128;",
        "__host__ inline int bin_fpt(int64_t n) { return n < 256 * 1024 ? 1 : n < 1024 * 1024 ? 2 : 4; }",
        "c[j] = tid * SCAN_BATCH + j < n ? c[j] + (c[j] >> 2) + SEG_SLACK : 0u;",
        "fb.base = (int64_t)blockIdx.x * (256 * FPT);",
        "fb.view = (int)(fb.base / F);",
        "const bool big = fb.touched[it] > BIG_RECT;",
        "if (q < (uint32_t)BIG_MAX) {",
        "if (w.lds && fb.mine[it] && !big) {",
        "auto limit = [&](uint32_t tile) { if constexpr (SEG) return min(seg[tile + 1], o.capacity); else return o.capacity; };",
        "if constexpr (SEG) bin = first + c <= limit(tile) ? first : SEG_FULL;",
    ],
    "dmr_tri.hip": ["full |= (e > p.tile_offset[t + 1] || e > p.list_capacity) ? 1u : 0u;"],
    "dmr_api.hip": [
        "uint64_t placement_capacity(uint64_t R, int ntiles) { return R + R / 4 + (uint64_t)dmr::SEG_SLACK * (uint64_t)ntiles; }",
        "int size_bucket(size_t BF) { int b = 0; while ((BF >> (b + 1)) != 0) b++; return b; }",
        "bool placement_eligible(bool tet, const Dims& d) { return !tet && d.ntiles <= dmr::SCAN_SINGLE_MAX; }",
    ],
}


def test_constants_restated_as_the_kernels_have_them():
    for name, lines in RESTATED.items():
        text = open(os.path.join(CSRC, name)).read()
        for line in lines:
            assert text.count(line) == 1, (name, line)
    assert (PC.SEG_SLACK, PC.BIG_RECT, PC.BIG_MAX, PC.LDS_HIST_MAX, PC.SCAN_SINGLE_MAX, PC.MASK_CHUNK) == (32, 256, 128, 8192, 8192, 128)
    assert (PC.FPT_2, PC.FPT_4) == (256 * 1024, 1024 * 1024)
    assert [PC.seg_len(c) for c in (0, 3, 4, 20, 1000)] == [32, 35, 37, 57, 1282]
    assert PC.placed_capacity(42646, 1024) == 42646 + 10661 + 32768
    assert [PC.size_bucket(n) for n in (1, 2, 3, 6588, 262144)] == [0, 1, 1, 12, 18]


def test_view_configurations_are_this_files_own():
    """Placements and size estimates are keyed by (B, W, H, rows, ...): every pair has its own, and no other test module
    names one of them (as `B, H, W` in a row, the way the suite's scene tables and tests write a view configuration)."""
    configs = list(PC.VIEW_CONFIGS.values())
    assert len(set(configs)) == len(configs) == len(PC.FIT) + len(PC.OVER)
    own = {"tri_placed_cases.py", "test_tri_placed_paths_cpu.py", "test_tri_placed_paths_gpu.py"}
    for path in sorted(glob.glob(os.path.join(HERE, "*.py"))):
        if os.path.basename(path) in own:
            continue
        text = open(path).read()
        for B, H, W, _ in configs:
            assert not re.search(rf"\b{B}, {H}, {W}\b", text), (os.path.basename(path), (B, H, W))


_seen = {}


def _case(oracle, name):
    """the pair's two oracle forwards and classify(), once"""
    if name not in _seen:
        a, b, (B, H, W), rows = PC.pair(name)
        ra, rb = (PC.Ref(oracle, d, B, H, W, rows, grads=False) for d in (a, b))
        c = PC.classify(ra.st, rb.st, B, ra.F, H, W)
        _seen[name] = (ra, rb, c)
        print(f"\n{name}: {PC.summary(c)}")
    return _seen[name]


@pytest.mark.parametrize("name", list(PC.FIT))
def test_fitting_pair_fits_and_reaches_its_route(oracle, name):
    ra, rb, c = _case(oracle, name)
    B, H, W, rows = PC.VIEW_CONFIGS[name]
    # THE condition of a fitting pair, from the oracle's counts alone: every list of B fits the segment A's count gives its tile
    assert int(c["overflows"].sum()) == 0 and bool((c["cB"] <= c["seg"]).all())
    # ... while the segments are partly filled and some tiles' counts differ from A's, up and down
    assert c["changed"] > 0 and c["gained_and_fits"] > 0 and 0.05 < c["fill"] < 0.95, PC.summary(c)
    assert c["RB"] > 0 and np.isfinite(rb.color).all() and np.isfinite(rb.depth).all()
    assert ra.F == rb.F and c["tiles"] <= PC.SCAN_SINGLE_MAX
    moved = float((rb.d["verts"] - ra.d["verts"]).abs().max())
    assert 0.0 < moved <= PC.JITTER_PX * PC.pixel(H) * 1.0001
    if name == "big_queue":   # one workgroup with more big faces than its queue holds: the cooperative AND the direct route
        big = rb.st.get("tiles_touched") > PC.BIG_RECT
        gaps = np.nonzero(np.concatenate([[True], ~big, [True]]))[0]
        assert int(np.diff(gaps).max()) - 1 >= 200, "a run of at least 200 consecutive big faces"
        assert c["tiles"] > PC.BIG_RECT and c["max_big_per_workgroup"] > PC.BIG_MAX and c["direct_big_faces"] >= 32
        assert c["entries"]["big_mixed"] > 0 and c["entries"]["window"] > 0, PC.summary(c)
    if name == "behind_camera":   # vertices off screen and behind every view's eye plane
        vh = th.cat([rb.d["verts"].double(), th.ones(rb.d["verts"].shape[0], 1, dtype=th.float64)], dim=1)
        clip = th.einsum("bij,pj->bpi", rb.d["proj_mats"].double() @ rb.d["mv_mats"].double(), vh)
        w = clip[..., 3]
        assert bool((w < 0).any(dim=1).all()) and bool((w > 0).any(dim=1).all())
        assert float((clip[..., 0].abs() / w.abs()).max()) > 3.0, "vertices far off screen"
        assert c["straddles"] and c["entries"]["direct"] > 0
    if name == "bitonic_in_segments":
        assert c["sort"]["bitonic"] >= 1 and c["chunks"] > 16 and c["longest"] > PC.SORT_LDS_KEYS, PC.summary(c)
        assert c["tiles"] <= 8, "few tiles"
    if name == "tiles_8192":
        assert c["tiles"] == PC.SCAN_SINGLE_MAX and 0 < int((c["cB"] > 0).sum()) < c["tiles"] // 2
    if name == "straddle":
        assert B == 3 and ra.F % 256 != 0 and c["straddles"] and c["entries"]["direct"] > 0
        assert float(rb.d["bg"].abs().min()) > 0.0, "the case over a background"
    if name == "fpt2":
        assert c["fpt"] == 2 and PC.FPT_2 <= c["BF"] < PC.FPT_4 and c["tiles"] // B <= 16 and c["straddles"]
    if name == "fpt4":
        assert c["fpt"] == 4 and c["BF"] >= PC.FPT_4 and c["tiles"] // B <= 16
    if name not in ("fpt2", "fpt4"):
        assert c["fpt"] == 1
    if name == "band":   # a strict sub-band whose edges faces cross: fewer entries than the full frame's, rows outside untouched
        gy = (H + 15) // 16
        assert 0 < rows[0] < rows[1] < gy
        full = PC.Ref(oracle, rb.d, B, H, W, (0, 0), grads=False)
        gx = (W + 15) // 16
        cfull = full.st.get("ranges").reshape(-1, 2).astype(np.int64)
        cfull = (cfull[:, 1] - cfull[:, 0]).reshape(gy, gx)
        cband = c["cB"].reshape(gy, gx)
        assert 0 < c["RB"] < full.st.num_rendered
        assert bool((cband[:rows[0]] == 0).all()) and bool((cband[rows[1]:] == 0).all())
        assert bool((cband[rows[0]:rows[1]] == cfull[rows[0]:rows[1]]).all())
        # faces cross the band's edges: the rows just outside hold faces that the edge rows inside hold too
        assert cfull[rows[0] - 1].sum() > 0 and cfull[rows[1]].sum() > 0
        t_band, t_full = rb.st.get("tiles_touched"), full.st.get("tiles_touched")
        assert int(((t_band > 0) & (t_band < t_full)).sum()) > 0, "faces cut by the band"


@pytest.mark.parametrize("name", list(PC.OVER))
def test_overflow_pair_overflows_through_its_route(oracle, name):
    ra, rb, c = _case(oracle, name)
    B, H, W, _ = PC.VIEW_CONFIGS[name]
    route = PC.OVER[name][5]
    over = c["overflows"]
    assert bool((over == (c["cB"] > c["cA"] + c["cA"] // 4 + 32)).all())
    # the intended route delivers entries to overflowing tiles
    assert c["overflow_tiles"][route] >= 1 and c["entries"][route] > 0, PC.summary(c)
    if name == "over_window":
        assert c["big"] == 0 and not c["straddles"] and c["overflow_tiles"]["window"] == int(over.sum())
    if name == "over_cooperative":
        assert 0 < c["max_big_per_workgroup"] < PC.BIG_MAX and c["direct_big_faces"] == 0 and c["overflow_tiles"]["cooperative"] == int(over.sum())
    if name == "over_direct_big":
        assert c["max_big_per_workgroup"] > PC.BIG_MAX and c["direct_big_faces"] >= 32
    if name == "over_direct_view":
        assert B == 2 and c["straddles"] and c["big"] == 0
        stack = rb.st.get("tiles_touched").reshape(B, -1)[:, : 2 * PC.OVER[name][3]]
        assert bool((stack[1] > 0).all()), "view 1's copies are on screen"
        per, F = 256, ra.F
        assert (F // per) * per < F < (F // per + 1) * per, "the workgroup that holds view 0's last faces starts view 1"
    # no tile gains entries and still fits; every tile keeps its list or leaves its segment
    assert c["gained_and_fits"] == 0
    assert bool((c["cB"] >= c["cA"]).all()) and bool(((c["cB"] == c["cA"]) | over).all())
    # the kept tiles' lists are A's, entry for entry (F is equal and the stack comes first in both: face ids are the same)
    rA = ra.st.get("ranges").reshape(-1, 2).astype(np.int64)
    rB = rb.st.get("ranges").reshape(-1, 2).astype(np.int64)
    vA, vB = ra.st.get("values"), rb.st.get("values")
    kept = np.nonzero(~over & (c["cB"] > 0))[0]
    assert kept.shape[0] > 0
    for t in kept:
        assert np.array_equal(vA[rA[t, 0]:rA[t, 1]], vB[rB[t, 0]:rB[t, 1]]), t
    # overflowing tiles that were empty in A, overflowing tiles that were not, kept busy tiles next to an overflowing segment
    assert c["overflow_empty_in_A"] >= 1 and c["overflow_busy_in_A"] >= 1 and c["neighbours"] >= 1, PC.summary(c)
    # the same key: F equal, hence the same bucket of B * F
    assert ra.F == rb.F and PC.size_bucket(B * ra.F) == PC.size_bucket(B * rb.F) and c["fpt"] == 1
    # in A the stack lies beyond the far plane in every view
    assert int(ra.st.get("tiles_touched").reshape(B, -1)[:, : 2 * PC.OVER[name][3]].max()) == 0
    assert float(ra.d["verts"][: 4 * PC.OVER[name][3], 2].max()) == PC.FAR_Z
    # the pixels of the kept tiles render as in A: the oracle's image of B there is A's, bit for bit
    keep_px = ~PC.tile_pixels(over, B, H, W)
    assert np.array_equal(ra.color.transpose(0, 2, 3, 1)[keep_px], rb.color.transpose(0, 2, 3, 1)[keep_px])
