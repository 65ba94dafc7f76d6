"""The hit-parallel tri backward aggregates a tile's vertex-gradient rows in an LDS table of 560 slots
(k_tri_backward_hits, VTAB) and sends a row that finds no slot out with direct atomics.  Here single tiles are crowded
with far more distinct vertex rows than that -- 40 stacked 9 x 9 lattices (3 240 vertices) seen by one or a few 16 x 16
tiles -- so the table fills up and the fallback runs in the product build, not only under the ablation switch of
tests/test_fallback_gpu.py.  Gradients against the CPU oracle, at the parity bar of tests/test_tri_parity_gpu.py."""
import pytest
import torch as th

from dmesh_renderer_amd import scenes
from util import c_args, rel_err, upstream_grads

pytestmark = pytest.mark.gpu

GRAD_TOL = 1e-4
TABLE_SLOTS = 560

CASES = {
    # name: (layers, n, B, H, W)
    "one_tile": (40, 9, 1, 16, 16),
    "four_tiles_two_views": (40, 9, 2, 32, 32),
    "ragged_one_row": (30, 10, 1, 16, 40),
}


@pytest.mark.parametrize("case", list(CASES))
def test_backward_with_full_tables(oracle, hip_device, case):
    from dmesh_renderer_amd import _C
    L, n, B, H, W = CASES[case]
    d = scenes.layered_sheets(L, n, B, H, W, seed=5, opacity=(0.01, 0.05))
    assert d["verts"].shape[0] > 4 * TABLE_SLOTS
    sc = oracle.scene_from_module_inputs(d, H, W)
    _, _, ost = oracle.tri_forward(sc)
    gc, gd = upstream_grads(B, H, W)
    og = oracle.tri_backward(sc, ost, gc.numpy(), gd.numpy())
    args = c_args(d, hip_device)
    out = _C.render_tris(*args, H, W)
    assert out[0] == ost.num_rendered
    g = _C.render_tris_backward(*args, gc.to(hip_device), gd.to(hip_device), out[0], *out[3:7])
    th.cuda.synchronize()
    # the tiles really see more rows than the table holds: every vertex of the stacked lattices has a gradient
    touched = (abs(og["verts_color"]).sum(axis=1) > 0).sum()
    assert touched > 2 * TABLE_SLOTS, touched
    for got, key in zip(g, ("verts", "verts_color", "faces_opacity", "verts_depth", "faces_intense")):
        assert got.shape == og[key].shape
        e = rel_err(got.cpu().numpy(), og[key])
        assert e <= GRAD_TOL, f"{key}: {e}"
