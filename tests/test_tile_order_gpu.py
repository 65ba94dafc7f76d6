"""The tile order of placed calls (csrc/dmr_tile_order.hpp, build_placement in dmr_api.hip): blocks of neighbouring tiles
dealt to the 8 XCD classes instead of the exact path's "longest list first" over the frame.  The order is a matter of speed
only, so a placed call -- the second default call of a key, as in test_tri_placement_gpu.py -- must give what the exact
call before it gave: the same image bit for bit, the same lists, and gradients that differ by the order of the float
atomics alone.  Every view configuration here is used by no other test (the placement is keyed by it)."""
import numpy as np
import pytest
import torch as th

from dmesh_renderer_amd import scenes
from harness import capture_replay, replay
from test_tri_placement_gpu import GRAD_TOL, _exact, _launches, _speculative
from util import c_args, rel_err, upstream_grads

pytestmark = pytest.mark.gpu


def _scaled(L, n, B, H, W, seed, sx, sy):
    d = scenes.layered_sheets(L, n, B, H, W, seed=seed)
    d["verts"] = d["verts"] * th.tensor([sx, sy, 1.0])
    return d


# name: (scene, B, H, W, rows, asynchronous second call)
CASES = {
    "two_tiles": (lambda: scenes.layered_sheets(3, 12, 1, 16, 32, seed=31), 1, 16, 32, (0, 0), False),
    "nine_tiles": (lambda: scenes.layered_sheets(3, 14, 1, 48, 48, seed=32), 1, 48, 48, (0, 0), False),
    # 16 x 12 tiles in 4 x 3 blocks; the sheets leave 48 % of the tiles empty, the longest list has 304 entries (3 chunks)
    "half_empty": (lambda: scenes.layered_sheets(3, 40, 1, 192, 256, seed=33), 1, 192, 256, (0, 0), False),
    "two_views": (lambda: _scaled(3, 24, 2, 80, 112, 34, 1.5, 1.5), 2, 80, 112, (0, 0), False),
    "band": (lambda: _scaled(3, 24, 1, 80, 144, 35, 1.8, 1.8), 1, 80, 144, (1, 3), False),
    "asynchronous": (lambda: _scaled(3, 24, 1, 96, 176, 36, 1.5, 1.5), 1, 96, 176, (0, 0), True),
}


def _call(args, gcd, gdd, H, W, rows):
    from dmesh_renderer_amd import _C
    out, n = _launches(lambda: _C.render_tris(*args, H, W, rows=rows))
    g = _C.render_tris_backward(*args, gcd, gdd, out[0], *out[3:7], rows=rows)
    ex = lambda name: _C.export(name, args, False, out[0], out[3:7], H, W, th.int32).cpu().numpy()
    return out, n, [x.cpu().numpy() for x in g], ex("ranges"), ex("face_list")


@pytest.mark.parametrize("case", sorted(CASES))
def test_placed_call_equals_the_exact_call(hip_device, case):
    from dmesh_renderer_amd import _C
    make, B, H, W, rows, asynchronous = CASES[case]
    args = c_args(make(), hip_device)
    gc, gd = upstream_grads(B, H, W)
    gcd, gdd = gc.to(hip_device), gd.to(hip_device)
    redo0 = _C.redo_count()
    out0, n0, g0, ranges0, faces0 = _call(args, gcd, gdd, H, W, rows)
    assert _exact(n0), (case, n0)
    R = out0[0]
    assert R > 0
    if case == "half_empty":
        empty = float((ranges0.reshape(-1, 2)[:, 0] == ranges0.reshape(-1, 2)[:, 1]).mean())
        assert 0.4 <= empty <= 0.6, empty
    _C.overflowed()
    _C.set_async(asynchronous)
    try:
        out1, n1, g1, ranges1, faces1 = _call(args, gcd, gdd, H, W, rows)
        th.cuda.synchronize()
    finally:
        _C.set_async(False)
    assert _speculative(n1), (case, n1)
    assert not _C.overflowed() and _C.redo_count() == redo0
    assert out1[0] >= R if asynchronous else out1[0] == R  # (asynchronous: the capacity, an upper bound)
    assert th.equal(out1[1], out0[1]) and th.equal(out1[2], out0[2]), "the image must not depend on the tile order"
    np.testing.assert_array_equal(ranges1, ranges0)
    np.testing.assert_array_equal(faces1[:R], faces0)
    for a, b in zip(g1, g0):
        assert rel_err(a, b) <= GRAD_TOL


def test_graph_replay_of_the_placed_order(hip_device):
    from dmesh_renderer_amd import _C
    B, H, W = 1, 112, 208
    args = c_args(_scaled(3, 30, B, H, W, 37, 1.4, 1.4), hip_device)
    gc, gd = upstream_grads(B, H, W)
    gcd, gdd = gc.to(hip_device), gd.to(hip_device)

    def step():
        o = _C.render_tris(*args, H, W)
        return [o[1], o[2], *_C.render_tris_backward(*args, gcd, gdd, o[0], *o[3:7])]

    exact, n = _launches(step)
    assert _exact(n), n
    exact = [x.clone() for x in exact]
    graph, captured, eager = capture_replay(step, warmup=1)  # the warm-up call is placed already, and so is the captured one
    replay(graph, times=2)
    for got in (eager, captured):
        assert th.equal(got[0], exact[0]) and th.equal(got[1], exact[1])
        for a, b in zip(got[2:], exact[2:]):
            assert rel_err(a.cpu().numpy(), b.cpu().numpy()) <= GRAD_TOL
    _, n = _launches(lambda: _C.render_tris(*args, H, W))
    assert _speculative(n)
