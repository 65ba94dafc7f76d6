"""tri renderer, PLACED front end (k_project_verts with SegInit -> k_bin_faces -> k_tri_forward, whose workgroup 0 sums R and the
overflow bit from the cursors): the HIP path vs the CPU oracle on the scene pairs of tests/tri_placed_cases.py, one emission
route of bin_emit<FPT, true> after the other -- the window reservation, the cooperative emission of queued big faces, the
per-thread emission of another view's faces and of big faces beyond the queue, each with the per-tile slot limit
min(seg[t + 1], capacity) -- with one, two and four faces per thread, workgroups that straddle views, the bitonic sort inside
a padded segment, a frame of exactly 8 192 tiles, a band of rows and a background.  tests/test_tri_placed_paths_cpu.py
asserts, without a GPU, that each pair reaches its route and fits / leaves its segments.  Every test asserts which path ran:
its first call of the pair's view configuration the exact one, the calls it is about the placed one.

Fitting pairs: B binned into A's placement is the oracle's B -- R, tiles_touched, key_depth, ranges, face_list, n_contrib bit
for bit, colour / depth / final_T within 1e-5, the five gradients within 1e-4 (rel_err): BASELINE.json's bars.
Overflow pairs: the contract of an asynchronous call (dmr_binning.hip): a tile whose list left its segment renders as empty,
every other tile -- the neighbours of the overflowing segments included -- is the oracle's, the flag is raised, nothing is
stored behind a buffer; its backward is the oracle's with the upstream gradients of the empty tiles' pixels zeroed.  The
default call redoes such a frame once through the exact path and leaves a placement that fits.

MEASURED on the MI355X (every case prints its own figures, pytest -s).  Every index array, list and n_contrib exact; colour, depth
and final_T differ from the oracle's by 0.0 in every case, placed, asynchronous and redone; worst gradient error (rel_err) per case:
    big_queue 1.85e-06   behind_camera 8.68e-07   bitonic_in_segments 5.21e-07   tiles_8192 1.46e-06   straddle 1.16e-06
    fpt2 2.01e-06   fpt4 9.61e-07   band 1.05e-06
    over_window 1.46e-06   over_cooperative 1.55e-06   over_direct_big 1.97e-06   over_direct_view 1.79e-06  (asynchronous backward)
The 12 tests together 2.9 s, their oracle references included; slowest fpt4, 1.0 s (0.96 s of it the oracle), then big_queue 0.43 s.

MUTANTS (scratch builds, nothing of them in the tree; with every face id read from a list clamped into the mesh, since a slot
limit that is wrong lets a stale list slot through as a face id):
    cooperative route's limit = capacity    fails over_cooperative, over_direct_big (n_contrib of kept neighbour tiles); no older test
    direct route's limit = capacity         fails over_direct_view; no older test
    window accepts first < limit            fails over_window, over_direct_view; no older test
    size workgroup without its segment term fails all four overflow pairs; also five older tests (jump, async jump, graph, parity)
    k_build_placement without SEG_SLACK     fails tiles_8192, straddle, band (a redo); also four older placement / graph tests
    list_end returning e unconditionally    not run: k_tri_backward_pix has no capacity guard on such a list, a cursor behind the
                                            buffer would be read through
"""
import time

import numpy as np
import pytest
import torch as th

import capi_ctypes as capi
import tri_placed_cases as PC
from harness import GuardedTriCalls
from test_tri_placement_gpu import _exact, _launches, _speculative
from util import c_args, rel_err, upstream_grads

pytestmark = pytest.mark.gpu

FWD_TOL, GRAD_TOL = 1e-5, 1e-4
TRI_NAMES = ("verts", "verts_color", "faces_opacity", "verts_depth", "faces_intense")


def check_forward(_C, ref, args, R, color, depth, bufs, keep=None):
    """The call's lists and images against the oracle's: R, tiles_touched, key_depth on touched faces, ranges, face_list and
    n_contrib bit for bit; colour, depth and final_T within FWD_TOL (the per-pixel state on the rows of the call's band).
    keep (a [B, H, W] mask): only these pixels, and nothing of the lists.  -> (colour, depth, final_T errors)"""
    ost, B, H, W = ref.st, ref.B, ref.H, ref.W
    ex = lambda name, dtype: _C.export(name, args, False, R, bufs, H, W, dtype).cpu().numpy()
    if keep is None:
        assert R == ost.num_rendered
        np.testing.assert_array_equal(ex("tiles_touched", th.int32).view(np.uint32), ost.get("tiles_touched"))
        touched = ost.get("tiles_touched") > 0
        np.testing.assert_array_equal(ex("key_depth", th.float32).view(np.uint32)[touched], ost.get("depths").view(np.uint32)[touched])
        np.testing.assert_array_equal(ex("ranges", th.int32).view(np.uint32), ost.get("ranges"))
        np.testing.assert_array_equal(ex("face_list", th.int32).view(np.uint32), ost.get("values"))
        keep = np.ones((B, H, W), dtype=bool)
    y0, y1 = ref.band()
    band = np.zeros((B, H, W), dtype=bool)
    band[:, y0:y1] = True
    px = lambda a: a.reshape(B, H, W)[keep & band]
    np.testing.assert_array_equal(px(ex("n_contrib", th.int32).view(np.uint32)), px(ost.get("n_contrib")))
    et = float(np.abs(px(ex("final_T", th.float32)) - px(ost.get("final_T"))).max())
    ec = float(np.abs(color.cpu().numpy() - ref.color).transpose(0, 2, 3, 1)[keep].max())
    ed = float(np.abs(depth.cpu().numpy() - ref.depth)[:, 0][keep].max())
    assert max(ec, ed, et) <= FWD_TOL, (ec, ed, et)
    return ec, ed, et


def check_grads(ref, g, what=""):
    errs = [rel_err(got.cpu().numpy(), ref.grads[k]) for got, k in zip(g, TRI_NAMES)]
    assert max(errs) <= GRAD_TOL, (what, dict(zip(TRI_NAMES, errs)))
    return max(errs)


@pytest.mark.parametrize("name", list(PC.FIT))
def test_fitting_pair_is_binned_into_its_segments(oracle, hip_device, name):
    """A by default call: the exact path (the first call of this view configuration), which leaves the placement.  B by default
    call: the placed path, no redo, the oracle's B.  big_queue and bitonic_in_segments once more asynchronously: the same image
    bit for bit, no overflow, and the placement's capacity in R's place."""
    from dmesh_renderer_amd import _C
    t_start = time.perf_counter()
    a, b, (B, H, W), rows = PC.pair(name)
    ra = PC.Ref(oracle, a, B, H, W, rows, grads=False)
    rb = PC.Ref(oracle, b, B, H, W, rows)
    cls = PC.classify(ra.st, rb.st, B, ra.F, H, W)
    assert not cls["overflows"].any()
    t_oracle = time.perf_counter() - t_start
    aargs, bargs = c_args(a, hip_device), c_args(b, hip_device)
    _C.overflowed()
    out, n = _launches(lambda: _C.render_tris(*aargs, H, W, rows=rows))
    assert _exact(n), ("the first call of a view configuration takes the exact path: is it used elsewhere?", n)
    assert out[0] == cls["RA"]
    redo0 = _C.redo_count()
    out, n = _launches(lambda: _C.render_tris(*bargs, H, W, rows=rows))
    assert _speculative(n) and _C.redo_count() == redo0, n
    ec, ed, et = check_forward(_C, rb, bargs, out[0], out[1], out[2], out[3:7])
    g = _C.render_tris_backward(*bargs, rb.gc.to(hip_device), rb.gd.to(hip_device), out[0], *out[3:7], rows=rows)
    th.cuda.synchronize()
    eg = check_grads(rb, g, name)
    if name in PC.ASYNC_TOO:
        _C.set_async(True)
        try:
            again, n = _launches(lambda: _C.render_tris(*bargs, H, W, rows=rows))
        finally:
            _C.set_async(False)
        assert _speculative(n) and not _C.overflowed()
        assert again[0] == PC.placed_capacity(cls["RA"], cls["tiles"])
        assert th.equal(again[1], out[1]) and th.equal(again[2], out[2])
    assert _C.redo_count() == redo0 and not _C.overflowed()
    print(f"\n{name}: R {cls['RA']} -> {cls['RB']}, fill {cls['fill']:.2f}, fpt {cls['fpt']}, entries {cls['entries']}, sort {cls['sort']}, "
          f"chunks {cls['chunks']}; colour {ec:.2e}, depth {ed:.2e}, final_T {et:.2e}, gradients {eg:.2e}; "
          f"oracle {t_oracle:.2f} s, test {time.perf_counter() - t_start:.2f} s")


@pytest.mark.parametrize("name", list(PC.OVER))
def test_overflowing_segments_render_empty_and_are_redone(oracle, hip_device, name):
    """A by default call (exact: the placement, and the backward's estimate).  Then B
    asynchronously, through the C ABI with guard bytes behind every buffer: the guards intact, the flag raised, every pixel of
    a tile that kept its list the oracle's, every pixel of a tile that left its segment the background; its asynchronous
    backward the oracle's of B with the upstream gradients zeroed on those tiles (the backward is linear in them), no overflow
    of its own.  Then B by default call: binned, refuted, redone once through the exact path -- the oracle's, lists bit for bit;
    B again: placed, bit-identical; A again, whose lists fit B's segments: placed, the oracle's."""
    from dmesh_renderer_amd import _C
    t_start = time.perf_counter()
    a, b, (B, H, W), rows = PC.pair(name)
    ra = PC.Ref(oracle, a, B, H, W, grads=False)
    rb = PC.Ref(oracle, b, B, H, W, grads=False)
    cls = PC.classify(ra.st, rb.st, B, ra.F, H, W)
    over_px = PC.tile_pixels(cls["overflows"], B, H, W)
    assert over_px.any() and not over_px.all() and cls["gained_and_fits"] == 0
    rz = PC.Ref(oracle, b, B, H, W, zero=over_px)   # B's gradients without the overflowing tiles' pixels
    t_oracle = time.perf_counter() - t_start
    calls = GuardedTriCalls(hip_device)
    lib, ASYNC = calls.lib, 1
    lib.dmr_overflowed(-1, 1)
    # ---- A: the exact path
    (RA, _, _, _), n = _launches(lambda: calls.forward(a, B, H, W, 0))
    assert _exact(n), ("the first call of a view configuration takes the exact path: is it used elsewhere?", n)
    assert RA == cls["RA"]
    calls.backward(a, B, H, W, 0, RA, rz.gc, rz.gd)
    assert not lib.dmr_overflowed(-1, 1)
    # ---- B, asynchronous: cannot redo
    (R, color, depth, args), n = _launches(lambda: calls.forward(b, B, H, W, ASYNC))   # (the guards are checked in there)
    assert _speculative(n), n
    assert lib.dmr_overflowed(-1, 1), "a list that left its segment must be flagged"
    assert R == PC.placed_capacity(cls["RA"], cls["tiles"])
    bufs = [calls.buffers[w] for w in (capi.BUF_POINT, capi.BUF_FACE, capi.BUF_BINNING, capi.BUF_IMAGE)]
    ec, ed, et = check_forward(_C, rb, args, R, color, depth, bufs, keep=~over_px)
    ex = lambda name_, dtype: _C.export(name_, args, False, R, bufs, H, W, dtype).cpu().numpy().reshape(B, H, W)
    bg = b["bg"].numpy()
    cnp, dnp = color.cpu().numpy(), depth.cpu().numpy()
    for ch in range(3):
        assert bool((cnp[:, ch][over_px] == bg[ch]).all()), "an overflowing tile renders as background"
    assert bool((dnp[:, 0][over_px] == 1.0).all())
    assert bool((ex("n_contrib", th.int32)[over_px] == 0).all()) and bool((ex("final_T", th.float32)[over_px] == 1.0).all())
    full_gc, full_gd = upstream_grads(B, H, W)   # the whole upstream gradient: the empty tiles' share must come to nothing
    g = calls.backward(b, B, H, W, ASYNC, R, full_gc, full_gd)
    assert not lib.dmr_overflowed(-1, 1), "the record buffer, sized from A's pairs, holds B's without the overflowing tiles"
    eg = check_grads(rz, g, name + " async")
    # ---- B, default: refuted and redone once
    bargs, aargs = c_args(b, hip_device), c_args(a, hip_device)
    redo0 = _C.redo_count()
    out, n = _launches(lambda: _C.render_tris(*bargs, H, W))
    assert n["k_scatter_faces"] == 2 and _exact(n) and _C.redo_count() == redo0 + 1, n
    ec2, ed2, et2 = check_forward(_C, rb, bargs, out[0], out[1], out[2], out[3:7])
    again, n = _launches(lambda: _C.render_tris(*bargs, H, W))
    assert _speculative(n) and _C.redo_count() == redo0 + 1, n
    assert again[0] == out[0] and th.equal(again[1], out[1]) and th.equal(again[2], out[2])
    back, n = _launches(lambda: _C.render_tris(*aargs, H, W))
    assert _speculative(n) and _C.redo_count() == redo0 + 1, n
    ec3, ed3, et3 = check_forward(_C, ra, aargs, back[0], back[1], back[2], back[3:7])
    assert not _C.overflowed()
    print(f"\n{name}: R {cls['RA']} -> {cls['RB']}, overflowing tiles {int(cls['overflows'].sum())} of {cls['tiles']} "
          f"({cls['overflow_empty_in_A']} empty in A), by route {cls['overflow_tiles']}, neighbours {cls['neighbours']}; "
          f"async: colour {ec:.2e}, depth {ed:.2e}, final_T {et:.2e}, gradients {eg:.2e}; default: colour {max(ec2, ec3):.2e}, "
          f"depth {max(ed2, ed3):.2e}; oracle {t_oracle:.2f} s, test {time.perf_counter() - t_start:.2f} s")
