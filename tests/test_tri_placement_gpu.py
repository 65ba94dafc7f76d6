"""Speculative placement of the tile segments (tri forward, frames up to 8 192 tiles; dmr_api.hip "Speculative PLACEMENT"):
after the first call of a key the front end is projection -> ONE binning kernel that emits straight into segments placed
from the previous counts (+ 25 % + 32 entries per tile).  Every view configuration here is used by no other test: the
placement, like the size estimates, is keyed by it."""
import os
import sys
import tempfile

import numpy as np
import pytest
import torch as th

from dmesh_renderer_amd import scenes
from harness import HERE, GuardedTriCalls, _run_child, capture_replay, replay
from util import c_args, rel_err, upstream_grads

pytestmark = pytest.mark.gpu
FWD_TOL, GRAD_TOL = 1e-5, 1e-4
TRI_NAMES = ("verts", "verts_color", "faces_opacity", "verts_depth", "faces_intense")
SLACK = 32  # dmr_kernels.hpp, SEG_SLACK


def _launches(fn):
    """fn() with the per-stage profile on -> (fn's result, {stage name: launches})."""
    from dmesh_renderer_amd import _C
    _C.profile_collect()
    _C.profile_enable(0xfff)
    try:
        r = fn()
        th.cuda.synchronize()
        _, n = _C.profile_collect()
    finally:
        _C.profile_enable(0)
    return r, {_C.stage_name(i): int(k) for i, k in enumerate(n)}


def _speculative(n):
    return n["k_setup_faces"] == 0 and n["k_scan_tiles"] == 0 and n["k_scatter_faces"] == 1


def _exact(n):
    return n["k_setup_faces"] >= 1 and n["k_scan_tiles"] >= 1


# ---- (a) a mesh that drifts ---------------------------------------------------------------------------------------------------
DRIFT = (1, 304, 368)
PIXEL = 2.0 * 3.0 * 0.57735 / DRIFT[1]  # world units per pixel at the cameras' distance (radius 3, fovy 60 deg)


def drift_scene(step):
    """Three 48 x 48 sheets scaled beyond the frame (no silhouette inside it: every tile is busy, ~10-14 px faces), the
    vertices of step > 0 jittered by up to +- 2 pixels in x and y around their place.  A tile of c entries can gain at
    most the faces whose bounding box lies within the jitter of touching it, ~0.7 c for these sizes; c + 0.7 c stays
    inside c + c / 4 + 32 up to c = 71, and these tiles hold 20-60."""
    B, H, W = DRIFT
    d = scenes.layered_sheets(3, 48, B, H, W, seed=21)
    v = d["verts"].clone()
    v[:, :2] *= 2.6
    if step:
        g = th.Generator().manual_seed(100 + step)
        v[:, :2] += (th.rand(v.shape[0], 2, generator=g) * 2.0 - 1.0) * (2.0 * PIXEL)
    d["verts"] = v
    return d


def test_drifting_mesh_is_binned_speculatively_and_bit_identical(hip_device):
    from dmesh_renderer_amd import _C
    B, H, W = DRIFT
    steps = 5
    with tempfile.TemporaryDirectory() as tmp:
        for k in range(steps):  # every step as the first call of a fresh process: the exact path
            _run_child([sys.executable, os.path.join(HERE, "placement_child.py"), str(k), os.path.join(tmp, f"{k}.npy")],
                       "placement child ok", 240)
        redo = None
        for k in range(steps):
            args = c_args(drift_scene(k), hip_device)
            out, n = _launches(lambda: _C.render_tris(*args, H, W))
            assert _exact(n) if k == 0 else _speculative(n), (k, n)
            if k == 0:
                redo = _C.redo_count()
            got = np.concatenate([out[1].cpu().numpy().reshape(-1), out[2].cpu().numpy().reshape(-1)])
            ref = np.load(os.path.join(tmp, f"{k}.npy"))
            assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), k
        assert _C.redo_count() == redo, "no call after the first may have been redone"


# ---- (b) a jump ---------------------------------------------------------------------------------------------------------------
def _half(side, B, H, W, seed):
    d = scenes.layered_sheets(3, 20, B, H, W, seed=seed)
    d["verts"] = d["verts"] * th.tensor([0.5, 1.0, 1.0]) + th.tensor([0.8 * side, 0.0, 0.0])
    return d


def test_jump_into_empty_tiles_is_redone_once(hip_device, oracle):
    from dmesh_renderer_amd import _C
    B, H, W = 1, 296, 376
    left, right = _half(-1.0, B, H, W, 4), _half(1.0, B, H, W, 5)
    _C.render_tris(*c_args(left, hip_device), H, W)
    args = c_args(right, hip_device)
    sc = oracle.scene_from_module_inputs(right, H, W)
    oc, od, ost = oracle.tri_forward(sc)
    redo0 = _C.redo_count()
    out, n = _launches(lambda: _C.render_tris(*args, H, W))
    assert n["k_scatter_faces"] == 2 and _exact(n), n  # the binning kernel, then the exact path
    assert _C.redo_count() == redo0 + 1
    assert out[0] == ost.num_rendered
    assert np.abs(out[1].cpu().numpy() - oc).max() <= FWD_TOL and np.abs(out[2].cpu().numpy() - od).max() <= FWD_TOL
    again, n = _launches(lambda: _C.render_tris(*args, H, W))  # the redo refreshed the placement
    assert _speculative(n) and _C.redo_count() == redo0 + 1
    assert th.equal(again[1], out[1]) and th.equal(again[2], out[2]) and again[0] == out[0]


def test_async_jump_is_clamped_and_flagged(hip_device, oracle):
    """Through the C ABI with an allocator of its own: every buffer is followed by guard words.  The asynchronous call of
    the second mesh must raise the overflow word and leave the guards alone; the default call then repairs it."""
    calls = GuardedTriCalls(hip_device)
    lib = calls.lib
    B, H, W = 1, 280, 392
    forward = lambda d, flags: calls.forward(d, B, H, W, flags)

    left, right = _half(-1.0, B, H, W, 6), _half(1.0, B, H, W, 7)
    lib.dmr_overflowed(-1, 1)
    forward(left, 0)                       # exact path: leaves the placement
    assert not lib.dmr_overflowed(-1, 1)
    forward(right, 1)                      # DMR_FLAG_ASYNC: cannot redo
    assert lib.dmr_overflowed(-1, 1), "the jump must be flagged"
    redo0 = lib.dmr_redo_count()
    R, color, depth, _ = forward(right, 0)
    assert lib.dmr_redo_count() == redo0 + 1 and not lib.dmr_overflowed(-1, 1)
    oc, od, ost = oracle.tri_forward(oracle.scene_from_module_inputs(right, H, W))
    assert R == ost.num_rendered
    assert np.abs(color.cpu().numpy() - oc).max() <= FWD_TOL and np.abs(depth.cpu().numpy() - od).max() <= FWD_TOL
    R2, color2, depth2, _ = forward(right, 1)  # now it fits: the asynchronous call is the default call's image
    assert not lib.dmr_overflowed(-1, 1) and R2 >= R
    assert th.equal(color2, color) and th.equal(depth2, depth)


# ---- (c) a scene that shrinks -------------------------------------------------------------------------------------------------
def test_shrinking_scene_refreshes_the_placement(hip_device):
    """A default call whose R is below half the R its placement was built from drops the placement; the next default call
    rebuilds it through the exact path (no redo).  Seen from outside: the capacity an asynchronous call reports."""
    from dmesh_renderer_amd import _C
    B, H, W = 1, 312, 360
    ntiles = ((H + 15) // 16) * ((W + 15) // 16)
    big = scenes.layered_sheets(4, 30, B, H, W, seed=9)  # four sheets that cover the whole frame
    big["verts"] = big["verts"] * th.tensor([2.6, 2.6, 1.0])
    small = dict(big)  # the three far sheets leave through the far plane: what stays is a subset of every tile's list
    small["verts"] = big["verts"].clone()
    small["verts"][: 3 * 30 * 30, 2] = -20.0
    abig, asmall = c_args(big, hip_device), c_args(small, hip_device)

    def capacity(args):
        _C.set_async(True)
        try:
            r = _C.render_tris(*args, H, W)[0]
            th.cuda.synchronize()
        finally:
            _C.set_async(False)
        assert not _C.overflowed()
        return r

    _C.overflowed()
    Rbig = _C.render_tris(*abig, H, W)[0]
    redo0 = _C.redo_count()
    assert capacity(asmall) == Rbig + Rbig // 4 + SLACK * ntiles
    o, n = _launches(lambda: _C.render_tris(*asmall, H, W))
    Rsmall = o[0]
    assert _speculative(n) and 2 * Rsmall < Rbig
    o2, n = _launches(lambda: _C.render_tris(*asmall, H, W))
    assert _exact(n), "the stale placement must have been dropped"
    assert th.equal(o2[1], o[1]) and o2[0] == Rsmall
    assert capacity(asmall) == Rsmall + Rsmall // 4 + SLACK * ntiles
    _, n = _launches(lambda: _C.render_tris(*asmall, H, W))
    assert _speculative(n)
    assert _C.redo_count() == redo0


# ---- (d) num_rendered and the exports on the speculative path ---------------------------------------------------------------------
def test_speculative_path_reports_the_oracles_lists(hip_device, oracle):
    from dmesh_renderer_amd import _C
    B, H, W = 2, 288, 384
    gc, gd = upstream_grads(B, H, W)
    first = scenes.layered_sheets(3, 24, B, H, W, seed=12)
    d = dict(first)
    d["verts"] = first["verts"] + (th.rand(first["verts"].shape, generator=th.Generator().manual_seed(3)) - 0.5) * 0.01
    _C.render_tris(*c_args(first, hip_device), H, W)
    sc = oracle.scene_from_module_inputs(d, H, W)
    oc, od, ost = oracle.tri_forward(sc)
    og = oracle.tri_backward(sc, ost, gc.numpy(), gd.numpy())
    args = c_args(d, hip_device)
    redo0 = _C.redo_count()
    out, n = _launches(lambda: _C.render_tris(*args, H, W))
    assert _speculative(n) and _C.redo_count() == redo0
    assert out[0] == ost.num_rendered
    ex = lambda name, dt: _C.export(name, args, False, out[0], out[3:7], H, W, dt).cpu().numpy()
    np.testing.assert_array_equal(ex("tiles_touched", th.int32).view(np.uint32), ost.get("tiles_touched"))
    np.testing.assert_array_equal(ex("ranges", th.int32).view(np.uint32), ost.get("ranges"))
    np.testing.assert_array_equal(ex("face_list", th.int32).view(np.uint32), ost.get("values"))
    np.testing.assert_array_equal(ex("n_contrib", th.int32).view(np.uint32), ost.get("n_contrib"))
    assert np.abs(out[1].cpu().numpy() - oc).max() <= FWD_TOL and np.abs(out[2].cpu().numpy() - od).max() <= FWD_TOL
    g = _C.render_tris_backward(*args, gc.to(hip_device), gd.to(hip_device), out[0], *out[3:7])
    for got, k in zip(g, TRI_NAMES):
        assert rel_err(got.cpu().numpy(), og[k]) <= GRAD_TOL, k


# ---- (e) HIP graph -------------------------------------------------------------------------------------------------------------
def test_graph_replays_the_speculative_path(hip_device, oracle):
    """Forward + backward captured behind two warm-up calls (the second one already speculative); the mesh then moves a little
    in place and the replay must give the new scene's image and gradients: the placement lives at fixed addresses."""
    from dmesh_renderer_amd import _C
    B, H, W = 1, 272, 400
    d = scenes.layered_sheets(3, 24, B, H, W, seed=14)
    gc, gd = upstream_grads(B, H, W)
    gcd, gdd = gc.to(hip_device), gd.to(hip_device)
    args = c_args(d, hip_device)

    def step():
        o = _C.render_tris(*args, H, W)
        return [o[1], o[2], *_C.render_tris_backward(*args, gcd, gdd, o[0], *o[3:7])]

    graph, captured, eager = capture_replay(step, warmup=2)
    replay(graph)
    assert th.equal(captured[0], eager[0]) and th.equal(captured[1], eager[1])
    moved = dict(d)
    moved["verts"] = d["verts"] + (th.rand(d["verts"].shape, generator=th.Generator().manual_seed(5)) - 0.5) * 0.01
    args[1].copy_(moved["verts"].to(hip_device))
    replay(graph, times=2)
    sc = oracle.scene_from_module_inputs(moved, H, W)
    oc, od, ost = oracle.tri_forward(sc)
    og = oracle.tri_backward(sc, ost, gc.numpy(), gd.numpy())
    assert np.abs(captured[0].cpu().numpy() - oc).max() <= FWD_TOL and np.abs(captured[1].cpu().numpy() - od).max() <= FWD_TOL
    for got, k in zip(captured[2:], TRI_NAMES):
        assert rel_err(got.cpu().numpy(), og[k]) <= GRAD_TOL, k
    _, n = _launches(lambda: _C.render_tris(*args, H, W))
    assert _speculative(n)
