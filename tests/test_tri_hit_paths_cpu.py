"""The tri edge scenes of tests/tri_hit_cases.py reach what they are for -- asserted on the CPU oracle and the float64 model
alone, with the rules of dmr_tri.hip and dmr_kernels.hpp restated by tri_hit_cases.classify -- the constants that restatement
rests on are still in the sources as text, and on every scene the model agrees with the oracle on the four gradients the
reference renderer computes exactly (so the model is pinned on these scenes before the GPU is asked, faces of opacity 1 and
pixels that stop early included).  A kernel threshold that moves fails here until the table follows."""
import os

import numpy as np
import pytest

import grad_cases
import tri_hit_cases as HC
from util import rel_err

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dmesh_renderer_amd", "csrc")

# The lines tri_hit_cases restates, each once in its file.
RESTATED = {
    "dmr_tri.hip": [
        "constexpr int VTAB = 560;   // vertex-row slots per workgroup",
        "constexpr int TAB_PROBES = 16;",
        "for (uint32_t g0 = 0; g0 < ngroups; g0 += 256u) {",
        "const uint32_t ngroups = nrec / (uint32_t)HIT_GROUP;",
        "cp[i] = (c[i] + (uint32_t)(HIT_GROUP - 1)) & ~(uint32_t)(HIT_GROUP - 1);",
        "if (T < T_EPS) { done = true; break; }  // blend first, test after (Q9)",
        "if (alpha == 1.0f) {",
        "constexpr int Q = N / 4, ROWS = 1024 / Q;",
        "for (; t + 3 * ROWS < tiles; t += 4 * ROWS) {",
        "for (; t < tiles; t += ROWS) {",
    ],
    "dmr_kernels.hpp": ["constexpr int HIT_GROUP = 4;"],
    "dmr_device.hpp": ["constexpr float T_EPS = 0.0001f;    // auxiliary.h:8", "constexpr int TILE = 16;"],
    "dmr_api.hip": [
        "if (camera) dmr::launch_camera_reduce(s->B, d.gx * d.gy, 32, cam_part, cam_out, st);",
        "if (cam_out) dmr::launch_camera_reduce(s->B, band_tiles, 64, cam_part, cam_out, st);",
    ],
}


def test_constants_restated_as_the_kernels_have_them():
    for name, lines in RESTATED.items():
        text = open(os.path.join(CSRC, name)).read()
        for line in lines:
            assert text.count(line) == 1, (name, line)
    assert (HC.VTAB, HC.TAB_PROBES, HC.HIT_GROUP, HC.ROUND_GROUPS, HC.ROUND_RECORDS, HC.TILE) == (560, 16, 4, 256, 1024, 16)
    assert HC.T_EPS == 1e-4 and np.float32(HC.T_EPS) == np.float32(0.0001)
    assert (HC.TRI_N, HC.TET_N) == (32, 64)
    assert (HC.reduce_rows(32), HC.reduce_rows(64)) == (128, 64)
    # some thread row runs the unrolled loop above 3 * ROWS tiles (384 / 192), every one above 4 * ROWS - 1 (511 / 255)
    assert [HC.reduce_unrolled_from(N) for N in (32, 64)] == [385, 193]
    assert [HC.reduce_unrolled_all(N) for N in (32, 64)] == [512, 256]


def test_reduce_thresholds_are_the_loops():
    """k_tri_camera_reduce's two loops replayed per thread row: with how many tiles which rows take the unrolled one."""
    def unrolled_rows(N, tiles):
        R = HC.reduce_rows(N)
        return sum(1 for j in range(R) if j + 3 * R < tiles)
    for N in (HC.TRI_N, HC.TET_N):
        R = HC.reduce_rows(N)
        assert unrolled_rows(N, HC.reduce_unrolled_from(N) - 1) == 0 and unrolled_rows(N, HC.reduce_unrolled_from(N)) == 1
        assert unrolled_rows(N, HC.reduce_unrolled_all(N) - 1) == R - 1 and unrolled_rows(N, HC.reduce_unrolled_all(N)) == R


def test_stacked_copies_keep_positions_and_take_new_ids():
    from dmesh_renderer_amd import scenes
    base = scenes.layered_sheets(2, 3, 2, 16, 16, seed=5, opacity=HC.CROWDED_OPACITY)
    c = 3
    d = HC.stacked(base, c)
    P, F = base["verts"].shape[0], base["faces"].shape[0]
    assert d["verts"].shape == (c * P, 3) and d["faces"].shape == (c * F, 3) and d["faces"].dtype == base["faces"].dtype
    assert d["verts_color"].shape == (c * P, 3) and d["faces_opacity"].shape == (c * F,)
    assert d["faces_intense"].shape == (2, c * F) and d["verts_depth"].shape == (2, c * P)
    for i in range(c):
        assert bool((d["verts"][i * P:(i + 1) * P] == base["verts"]).all())
        assert bool((d["verts_depth"][:, i * P:(i + 1) * P] == base["verts_depth"]).all())
        assert bool((d["faces"][i * F:(i + 1) * F] == base["faces"] + i * P).all())   # face copy i on vertex copy i
        assert sorted(d["faces_opacity"][i * F:(i + 1) * F].tolist()) == sorted(base["faces_opacity"].tolist())
    assert not bool((d["verts_color"][:P] == d["verts_color"][P:2 * P]).any())          # fresh colours per copy
    assert float(d["faces_opacity"].max()) <= HC.CROWDED_OPACITY[1]


_seen = {}


def _case(oracle, name):
    if name not in _seen:
        r = HC.reference(oracle, name)
        _seen[name] = r.classify()
        print(f"\n{name}: {HC.summary(_seen[name])}  factor {r.factor:g}  "
              f"max|model| {({k: float(np.abs(v).max()) for k, v in r.grads.items()})}")
    return _seen[name]


@pytest.mark.parametrize("name", list(HC.CASES))
def test_case_reaches_what_it_is_for(oracle, name):
    c = _case(oracle, name)
    assert c["kept"] >= 0.8, c["kept"]
    assert c["pairs"] > 0
    if name in HC.CROWDED:
        # one tile holds both: more distinct vertex rows among the faces its kept pixels blend than twice the table's slots
        # (so most rows are refused and leave through direct atomics) and at least four rounds of records
        both = (c["rows_blended"] > 2 * HC.VTAB) & (c["rounds"] >= 4)
        assert both.any(), HC.summary(c)
        assert (c["rows"] >= c["rows_blended"]).all() and (c["list"].max() > HC.ROUND_RECORDS)
        assert c["T_zero"] == 0 and c["T_below_eps"] == 0, HC.summary(c)   # nothing here stops early: that is the opaque cases'
    if name in HC.OPAQUE:
        assert c["T_zero"] >= 500 and c["T_below_eps"] >= 200, HC.summary(c)
    if name in HC.WIDE:
        assert c["tiles_per_view"] > 4 * HC.reduce_rows(HC.TRI_N) - 1, c["tiles_per_view"]
        B, H, W = HC.CASES[name][2:5]
        assert H % HC.TILE == 1 and W % HC.TILE == 9     # the last tile row is one pixel high, the last column nine wide
        assert c["tiles"] == B * c["tiles_per_view"]


@pytest.mark.parametrize("name", list(HC.TET_WIDE))
def test_tet_wide_reaches_the_unrolled_reduce(name):
    m, B, H, W, op, seed = HC.TET_WIDE[name]
    per_view = ((H + HC.TILE - 1) // HC.TILE) * ((W + HC.TILE - 1) // HC.TILE)
    assert per_view > 4 * HC.reduce_rows(HC.TET_N) - 1, per_view
    assert H % HC.TILE == 1 and W % HC.TILE == 9
    assert max(v[2] * v[3] for v in grad_cases.TET_CASES.values()) < H * W   # larger than any frame of the tet model tests
    assert per_view <= 3 * HC.reduce_rows(HC.TRI_N)   # (no substitute for the tri `wide` cases: N = 32 needs more than 511)


@pytest.mark.parametrize("name", list(HC.TET_WIDE))
def test_tet_wide_model_keeps_enough(oracle, name):
    """TetCameraGradRef keeps at least 0.8 of the frame (grad_cases.reference asserts it) and its matrix gradients are at
    least 1, so MATS_TOL is a relative bar on these frames."""
    d, B, H, W, seed, ref, gc, gd, rg = HC.tet_reference(oracle, name)
    big = {k: float(np.abs(rg[k]).max()) for k in ("mv_mats", "proj_mats")}
    print(f"\n{name}: kept {ref.kept_fraction:.3f}  max|model| {big}")
    assert ref.kept_fraction >= 0.8
    assert min(big.values()) >= 1.0, big


@pytest.mark.parametrize("name", list(HC.CASES))
def test_model_agrees_with_oracle_on_the_exactly_computed_gradients(oracle, name):
    """verts_color, faces_opacity, verts_depth, faces_intense: the float64 model against oracle.tri_backward, rel_err <= 1e-4 with
    the reference's largest entry at least 1 (the scaled upstream sees to that)."""
    r = HC.reference(oracle, name)
    og = r.oracle_grads(oracle)
    for k in HC.EXACT_KEYS:
        big = float(np.abs(r.grads[k]).max())
        e = rel_err(og[k], r.grads[k])
        print(f"\n{name} {k}: oracle vs model {e:.2e}  (max|model| {big:.3g}, factor {r.factor:g})")
        assert big >= 1.0, (k, big)
        assert e <= 1e-4, (k, e)
    # and every one of the seven references is at least 1: the GPU file's bars are relative
    for k, v in r.grads.items():
        assert float(np.abs(v).max()) >= 1.0, k
    # the forward: the model's colour and depth are the oracle's on the pixels it keeps
    m = r.model
    oc = r.color[m.view.numpy(), :, m.py.numpy(), m.px.numpy()]
    od = r.depth[m.view.numpy(), 0, m.py.numpy(), m.px.numpy()]
    ec, ed = float(np.abs(oc - r.model_color.numpy()).max()), float(np.abs(od - r.model_depth.numpy()).max())
    print(f"{name}: forward colour {ec:.2e} depth {ed:.2e}")
    assert ec <= 1e-5 and ed <= 1e-5, (ec, ed)
