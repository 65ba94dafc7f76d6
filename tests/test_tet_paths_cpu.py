"""The tet edge scenes of tests/tet_cases.py reach what they are for -- asserted on the CPU oracle alone, with the rules of
dmr_sort.hpp, dmr_binning.hip, dmr_kernels.hpp and dmr_api.hip restated by tet_cases.classify -- and the constants that
restatement rests on are still in the sources as text.  A kernel threshold that moves fails here until the table follows."""
import os

import numpy as np
import pytest

import tet_cases as TC

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dmesh_renderer_amd", "csrc")

# The lines tet_cases restates, each once in its file.
RESTATED = {
    "dmr_sort.hpp": [
        "constexpr int SORT_LDS_KEYS = 2048;",
        "constexpr uint32_t SORT_NB_LOG2 = 6, SORT_NB = 1u << SORT_NB_LOG2, SORT_BUCKET_MAX = 96;",
        "if (n <= SORT_LDS_KEYS && n > 64u) {",
        "const uint32_t shift = bits > SORT_NB_LOG2 ? bits - SORT_NB_LOG2 : 0u;",
        "const uint32_t b = ((uint32_t)(mk[q] >> 32) - mn) >> shift;",
        "if (s_misc[2] <= SORT_BUCKET_MAX) {",
    ],
    "dmr_tet.hip": ["constexpr int FI_CHUNK = 256;"],
    "dmr_binning.hip": [
        "constexpr uint32_t BIG_RECT = 256;",
        "constexpr int BIG_MAX = 128;",
        "__host__ inline int bin_fpt(int64_t n) { return n < 256 * 1024 ? 1 : n < 1024 * 1024 ? 2 : 4; }",
        "const bool big = fb.touched[it] > BIG_RECT;",
        "if (q < (uint32_t)BIG_MAX) {",
    ],
    "dmr_kernels.hpp": [
        "constexpr int SCAN_SINGLE_MAX = 8192;",
        "inline bool sorts_own_tiles(const Dims& d) { return d.ntiles <= SCAN_SINGLE_MAX; }",
    ],
    "dmr_api.hip": ["uint64_t padded(uint64_t n) { return n + n / 4 + 4096; }"],
}


def test_constants_restated_as_the_kernels_have_them():
    for name, lines in RESTATED.items():
        text = open(os.path.join(CSRC, name)).read()
        for line in lines:
            assert text.count(line) == 1, (name, line)
    assert (TC.SORT_LDS_KEYS, TC.SORT_SMALL, TC.SORT_NB_LOG2, TC.SORT_BUCKET_MAX) == (2048, 64, 6, 96)
    assert (TC.FI_CHUNK, TC.BIG_RECT, TC.BIG_MAX, TC.SCAN_SINGLE_MAX) == (256, 256, 128, 8192)
    assert [TC.bin_fpt(n) for n in (1, 256 * 1024 - 1, 256 * 1024, 1024 * 1024 - 1, 1024 * 1024)] == [1, 1, 2, 2, 4]
    assert [TC.padded(n) for n in (0, 3, 16094)] == [4096, 4099, 24213]


def test_sort_path_at_its_thresholds():
    """The restated rule of sort_tile on keys made for it: the list lengths 64 / 65 and 2 048 / 2 049, a bucket of 96 / 97
    equal keys, a range narrower than the 64 buckets (shift 0), and the bucket shift at a range of 2^k."""
    u = lambda a: np.asarray(a, dtype=np.uint32)
    spread = lambda n: u(np.arange(n, dtype=np.int64) * 1000 + 5)
    assert TC.sort_path(spread(64)) == "segmented" and TC.sort_path(spread(65)) == "bucket"
    assert TC.sort_path(spread(2048)) == "bucket" and TC.sort_path(spread(2049)) == "bitonic"
    assert TC.sort_path(u([7] * 2049)) == "bitonic"
    # 100 keys 4 096 apart: range 99 * 4096, bit length 19, shift 13 -- two keys per bucket, and the copies of the first join bucket 0
    wide = u(np.arange(100, dtype=np.int64) * 4096 + 5)
    assert TC.sort_path(np.concatenate([wide, u([5] * 94)])) == "bucket"       # 96 keys in bucket 0
    assert TC.sort_path(np.concatenate([wide, u([5] * 95)])) == "segmented"    # 97
    assert TC.sort_path(u(list(range(40)) * 2)) == "bucket"                           # range 39 < 64: a bucket per value, 2 each
    assert TC.sort_path(u([3] * 97)) == "segmented"                                   # range 0: all in bucket 0
    # range 64 = 2^6: bit length 7, shift 1 -> buckets of two values: 48 keys at each of 0 and 1 share bucket 0 (96), one more tips it
    assert TC.sort_path(u([0] * 48 + [1] * 48 + [64])) == "bucket"
    assert TC.sort_path(u([0] * 48 + [1] * 49 + [64])) == "segmented"
    assert TC.sort_path(u([0] * 48 + [1] * 49 + [63])) == "bucket"                    # range 63: shift 0, they part


_seen = {}


def _case(oracle, name):
    """classify() and the image checks of a case, computed once (the forward only)."""
    if name not in _seen:
        r = TC.reference(oracle, name, grads=False)
        _seen[name] = dict(r.classify(), active=float(r.active.mean()), finite=bool(np.isfinite(r.color).all() and np.isfinite(r.depth).all()),
                           all_hit=bool((r.st.get("first_face") >= 0).all()))
        print(f"\n{name}: {_seen[name]}")
    return _seen[name]


@pytest.mark.parametrize("name", list(TC.CASES))
def test_case_reaches_what_it_is_for(oracle, name):
    c = _case(oracle, name)
    assert c["active"] > 0.2 and c["finite"], c
    assert c["R"] > 0 and c["longest"] > 0
    S = TC.SCAN_SINGLE_MAX
    if name == "tiles_8192":        # the last frame whose first-hit kernel sorts its own lists; the one-workgroup scan's slab full
        assert c["tiles"] == S and c["big"] > 0, c
    if name == "tiles_8320":        # k_tet_first_intersect<false>, k_sort_tiles, three-launch scan
        assert c["tiles"] > S and c["big"] > 0, c
    if name == "tiles_two_views":   # one view alone would not do it
        B = TC.CASES[name][1]
        assert c["tiles"] > S >= c["tiles"] // B and c["big"] > 0, c
    if name == "mixed_sorts":
        assert c["bucket"] >= 1 and c["segmented"] - c["small"] >= 1 and c["longest"] > TC.FI_CHUNK, c
    if name == "long_lists":
        assert c["segmented"] - c["small"] >= 1 and c["bitonic"] >= 1, c
    if name == "all_bitonic":
        assert c["bitonic"] == c["busy"] == c["tiles"] and c["chunks"] >= 25, c
    if name in TC.INSIDE:           # more big faces in one set-up workgroup than its queue holds: cooperative emission AND the fallback
        assert c["max_big_per_workgroup"] > TC.BIG_MAX and c["all_hit"], c
    if name == "inside_m7":         # long lists everywhere
        assert c["busy"] == c["tiles"] and c["small"] == 0 and c["longest"] > TC.FI_CHUNK, c
    if name == "fpt2":
        F = c["BF"] // TC.CASES[name][1]
        assert c["fpt"] == 2 and c["straddles"] and F % 512 != 0 and c["bitonic"] >= 1, c
    if name == "fpt4":
        assert c["fpt"] == 4 and c["BF"] >= TC.FPT_4 and c["bitonic"] >= 1, c
    if name not in ("fpt2", "fpt4"):
        assert c["fpt"] == 1
    if name in TC.SORT_CASES:       # equal depth keys -- Kuhn faces that share their nearest vertex -- on every path the case takes
        for path in ("bucket", "segmented", "bitonic"):
            assert c[path] == 0 or c["ties"][path] >= 1, (path, c)


@pytest.mark.parametrize("name", TC.INSIDE)
def test_camera_is_inside_the_mesh(name):
    """Every eye lies inside the scaled cube, and every view has vertices behind its eye plane (w < 0: mirrored by clamp_w)."""
    import torch as th
    d, B, H, W = TC.make(name)
    scale = TC.CASES[name][4]
    eyes = th.linalg.inv(d["mv_mats"].double())[:, :3, 3]
    assert float(eyes.abs().max()) < scale and float(d["verts"].abs().max()) == scale
    vh = th.cat([d["verts"].double(), th.ones(d["verts"].shape[0], 1, dtype=th.float64)], dim=1)
    w = th.einsum("bij,pj->bpi", d["proj_mats"].double() @ d["mv_mats"].double(), vh)[..., 3]
    assert bool((w < 0).any(dim=1).all()) and bool((w > 0).any(dim=1).all())


def test_band_case_is_a_proper_band(oracle):
    """tiles_8320 as rows (9, 41): still above SCAN_SINGLE_MAX tiles (the tile count does not depend on the band), fewer entries."""
    full = _case(oracle, TC.ROWS_CASE)
    r = TC.reference(oracle, TC.ROWS_CASE, rows=TC.ROWS, grads=False)
    c = r.classify()
    y0, y1 = r.band()
    assert (y0, y1) == (16 * TC.ROWS[0], 16 * TC.ROWS[1]) and y1 < r.H
    assert c["tiles"] == full["tiles"] and 0 < c["R"] < full["R"] and c["big"] > 0
    assert float(r.active[:, y0:y1].mean()) > 0.2 and float(np.abs(r.color[:, :, :y0]).max()) == 0.0 and float(np.abs(r.color[:, :, y1:]).max()) == 0.0


def test_redo_scene_refutes_its_size_guess(oracle):
    """The second scene of the redo test has more list entries than the capacity guessed from the first, by a margin."""
    R = {}
    longest = {}
    for scale in sorted(set(TC.REDO["scales"])):
        d = TC.redo_scene(scale)
        st = oracle.tet_forward(oracle.scene_from_module_inputs(d, TC.REDO["H"], TC.REDO["W"]))[3]
        R[scale], longest[scale] = st.num_rendered, int(st.get("n_contrib").max())
    small, big = (R[s] for s in sorted(R))
    print(f"\nredo scenes: R {small} and {big}, padded({small}) = {TC.padded(small)}, longest marches {longest}")
    assert big > 1.2 * TC.padded(small)
    assert TC.bin_fpt(TC.REDO["B"] * d["faces"].shape[0]) == 1
