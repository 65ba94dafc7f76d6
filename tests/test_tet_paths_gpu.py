"""tet renderer: HIP path vs the CPU oracle on the edge scenes of tests/tet_cases.py -- every binning, sort and first-hit path the
parity scenes of test_tet_parity_gpu.py never take (tests/test_tet_paths_cpu.py asserts, without a GPU, that each case does
take them): k_tet_first_intersect<false> behind k_sort_tiles and the three-launch scan (more than 8 192 tiles), the bitonic
network and the segmented rank sort inside k_tet_first_intersect<true>, first-hit walks of dozens of chunks, the cooperative
emission of big faces and its overflow past 128 per workgroup with tet keys, two and four faces per set-up thread with
workgroups that straddle views, a camera inside the mesh, and the redo of a refuted size guess in a tet forward.

The comparisons and bars are those of test_tet_parity_gpu.py: binning indices, the sorted lists and the march topology bit
for bit, forward 1e-5, gradients 1e-4 (rel_err), re-march vs march-sequence gradients 1e-5.

MEASURED on the MI355X (every case prints its own figures, pytest -s): every index array, list and topology array exact;
forward: colour <= 2.98e-07, depth <= 4.17e-07; gradients against the oracle <= 2.03e-06 (tiles_two_views); re-march vs
sequence backward <= 2.37e-06 (tiles_two_views; fpt2 2.38e-07, fpt4 3.82e-07 -- 1.31e-05 and 2.06e-05 before the sequence
kernel formed its hits from uncontracted sums, see test_backward_through_both_kernels).
Slowest test: 0.4 s (+ 0.3 s for its oracle reference), the 25 tests together 2.8 s.
"""
import time

import numpy as np
import pytest
import torch as th

import tet_cases as TC
from util import c_args, rel_err

pytestmark = pytest.mark.gpu

FWD_TOL = 1e-5
GRAD_TOL = 1e-4
SEQ_TOL = 1e-5
GRAD_KEYS = ("verts_color", "faces_opacity")


def _exports(_C, args, bufs, H, W, R):
    return lambda name, dtype: _C.export(name, args, True, R, bufs, H, W, dtype).cpu().numpy()


def check_forward(_C, ref, args, out, min_active=0.2):
    """What test_tet_parity_gpu.test_forward_and_topology asserts, for the rows of the call's band: the binning arrays, the sorted
    lists and the march topology bit for bit; colour and depth within FWD_TOL.  -> (colour error, depth error, R)"""
    ost, H, W = ref.st, ref.H, ref.W
    color, depth, active, bufs = out[0], out[1], out[2], out[3:7]
    ex = _exports(_C, args, bufs, H, W, ost.num_rendered)
    ranges = ex("ranges", th.int32).view(np.uint32)
    R = int(ranges.max()) if ranges.size else 0
    assert R == ost.num_rendered
    np.testing.assert_array_equal(ex("tiles_touched", th.int32).view(np.uint32), ost.get("tiles_touched"))
    touched = ost.get("tiles_touched") > 0
    np.testing.assert_array_equal(ex("key_depth", th.float32).view(np.uint32)[touched], ost.get("min_depths").view(np.uint32)[touched])
    np.testing.assert_array_equal(ex("max_depth", th.float32).view(np.uint32)[touched], ost.get("max_depths").view(np.uint32)[touched])
    np.testing.assert_array_equal(ranges, ost.get("ranges"))
    np.testing.assert_array_equal(ex("face_list", th.int32).view(np.uint32), ost.get("values"))
    y0, y1 = ref.band()
    rows = lambda a: a.reshape(ref.B, H, W)[:, y0:y1]   # (nothing writes the per-pixel state outside the band)
    for name in ("first_face", "first_tet", "last_face", "last_tet"):
        np.testing.assert_array_equal(rows(ex(name, th.int32)), rows(ost.get(name)), err_msg=name)
    np.testing.assert_array_equal(rows(ex("n_contrib", th.int32).view(np.uint32)), rows(ost.get("n_contrib")))
    np.testing.assert_array_equal(active.cpu().numpy(), ref.active)
    assert rows(ref.active).mean() > min_active, "scene must have marched pixels"
    ec = float(np.abs(color.cpu().numpy() - ref.color).max())
    ed = float(np.abs(depth.cpu().numpy() - ref.depth).max())
    assert ec <= FWD_TOL and ed <= FWD_TOL, (ec, ed)
    return ec, ed, R


def check_grads(ref, g, what=""):
    errs = [rel_err(got.cpu().numpy(), ref.grads[key]) for got, key in zip(g, GRAD_KEYS)]
    assert max(errs) <= GRAD_TOL, (what, dict(zip(GRAD_KEYS, errs)))
    return errs


def _seq_state(_C, args, bufs, H, W):
    """(longest march of the forward in steps, steps per pixel its march sequence had room for)"""
    longest, cap = _C.export("tet_seq", args, True, 0, bufs, H, W, th.int32).cpu().numpy().view(np.uint32)[:2]
    return int(longest), int(cap)


def _sort_launches(_C, call):
    """call() with the stage timers on -> (its result, launches of k_sort_tiles)"""
    th.cuda.synchronize()
    _C.profile_collect()
    _C.profile_enable(1 << _C.STAGE_SORT)
    try:
        out = call()
        th.cuda.synchronize()
    finally:
        _C.profile_enable(0)
    return out, int(_C.profile_collect()[1][_C.STAGE_SORT])


# One reference per case, shared by the case's tests (pytest runs a module-scoped parameter's tests together) and left unchanged.
@pytest.fixture(scope="module", params=list(TC.CASES))
def ref(request, oracle):
    t0 = time.perf_counter()
    r = TC.reference(oracle, request.param)
    r.name, r.cls = request.param, r.classify()
    print(f"\n{r.name}: oracle {time.perf_counter() - t0:.2f} s; {r.cls}")
    return r


def test_forward_and_topology(ref, hip_device):
    from dmesh_renderer_amd import _C
    args = c_args(ref.d, hip_device, tet=True)
    t0 = time.perf_counter()
    out, sorts = _sort_launches(_C, lambda: _C.render_tets(*args, ref.H, ref.W, 0))
    dt = time.perf_counter() - t0
    ec, ed, R = check_forward(_C, ref, args, out)
    # who sorted: above SCAN_SINGLE_MAX tiles k_sort_tiles, ahead of k_tet_first_intersect<false>; else the first-hit kernel itself
    assert (sorts >= 1) == (ref.cls["tiles"] > TC.SCAN_SINGLE_MAX), (sorts, ref.cls["tiles"])
    print(f"\n{ref.name}: R {R}, k_sort_tiles launches {sorts}, colour {ec:.2e}, depth {ed:.2e}, call {1e3 * dt:.1f} ms")


def test_backward_through_both_kernels(ref, hip_device):
    """Three calls of forward + backward: the first backward of the view configuration re-marches (k_tet_backward), the later ones
    consume the forward's march sequence (k_tet_backward_seq); the oracle's gradients each time, and the two paths agree.

    MEASURED on the MI355X: the two paths agree to 1.8e-07 .. 2.4e-06.  These cases found a defect: k_tet_backward_seq recomputed
    a hit's (t, u, v) with contracted arithmetic, and on the 20^3 lattices some rays graze a face (|den| = 4e-4 .. 2e-3 of
    |P||E1|, where float (u, v) is itself 2e-4 .. 9e-4 away from its double value): the paths differed by 1.31e-05 (fpt2) and
    2.06e-05 (fpt4).  The kernel now forms the hit from the forward's uncontracted sums (tet_hit, dmr_tet.hip)."""
    from dmesh_renderer_amd import _C
    args = c_args(ref.d, hip_device, tet=True)
    gc, gd = ref.gc.to(hip_device), ref.gd.to(hip_device)
    longest_march = int(ref.st.get("n_contrib").max())
    grads, worst = [], 0.0
    for call in range(3):
        out = _C.render_tets(*args, ref.H, ref.W, 0)
        g = _C.render_tets_backward(*args, gc, gd, *out[3:7])
        th.cuda.synchronize()
        longest, cap = _seq_state(_C, args, out[3:7], ref.H, ref.W)
        assert longest == longest_march
        if call == 0:
            assert cap == 0, "first backward of a view configuration: no estimate, the backward re-marches"
        else:
            assert 0 < longest <= cap, (longest, cap)  # the sequence is complete: k_tet_backward_seq did the work
        worst = max([worst] + check_grads(ref, g, f"call {call}"))
        grads.append([x.cpu().numpy() for x in g])
    # the topology and the lists the forward reports are unchanged by the sequence stores
    ex = _exports(_C, args, out[3:7], ref.H, ref.W, ref.st.num_rendered)
    np.testing.assert_array_equal(ex("n_contrib", th.int32).view(np.uint32), ref.st.get("n_contrib"))
    np.testing.assert_array_equal(ex("face_list", th.int32).view(np.uint32), ref.st.get("values"))
    seq = max(rel_err(a, b_) for a, b_ in zip(grads[0], grads[1]))
    print(f"\n{ref.name}: longest march {longest_march}, gradients {worst:.2e}, re-march vs sequence {seq:.2e}")
    assert seq <= SEQ_TOL, seq


@pytest.mark.parametrize("name", TC.INSIDE)
def test_inside_over_a_background(oracle, hip_device, name):
    """The camera inside the mesh once more over a non-zero background: a wrong T shows in the image."""
    from dmesh_renderer_amd import _C
    ref = TC.reference(oracle, name, bg=True, grads=False)
    assert float(ref.d["bg"].abs().min()) > 0.0
    args = c_args(ref.d, hip_device, tet=True)
    out = _C.render_tets(*args, ref.H, ref.W, 0)
    th.cuda.synchronize()
    ec, ed, _ = check_forward(_C, ref, args, out)
    # (no backward here: the first backward of this view configuration belongs to test_backward_through_both_kernels)
    print(f"\n{name} over a background: colour {ec:.2e}, depth {ed:.2e}")


def test_presorted_lists_in_a_band_of_rows(oracle, hip_device):
    """tiles_8320 as the band of tile rows (9, 41): k_sort_tiles and k_tet_first_intersect<false> with a grid that starts at row 9."""
    from dmesh_renderer_amd import _C
    ref = TC.reference(oracle, TC.ROWS_CASE, rows=TC.ROWS)
    args = c_args(ref.d, hip_device, tet=True)
    out, sorts = _sort_launches(_C, lambda: _C.render_tets(*args, ref.H, ref.W, 0, rows=TC.ROWS))
    assert sorts >= 1
    ec, ed, R = check_forward(_C, ref, args, out)
    y0, y1 = ref.band()
    assert float(out[0][:, :, :y0].abs().sum()) == 0.0 and float(out[0][:, :, y1:].abs().sum()) == 0.0
    g = _C.render_tets_backward(*args, ref.gc.to(hip_device), ref.gd.to(hip_device), *out[3:7], rows=TC.ROWS)
    th.cuda.synchronize()
    eg = check_grads(ref, g)
    print(f"\n{TC.ROWS_CASE} rows {TC.ROWS}: R {R}, colour {ec:.2e}, depth {ed:.2e}, gradients {max(eg):.2e}")


def _redo_refs(oracle):
    refs = {}
    for scale in sorted(set(TC.REDO["scales"])):
        refs[scale] = TC.Ref(oracle, TC.redo_scene(scale), TC.REDO["B"], TC.REDO["H"], TC.REDO["W"])
    return refs


def test_tet_size_guess_is_refuted_and_redone(oracle, hip_device):
    """Speculative sizing in a tet forward: the same shapes small on screen, then filling it -- R grows beyond the capacity
    guessed from the call before, the front end and the lists are enqueued again with a binning buffer of another size (the march
    sequence then lies at another offset; launch_tet_prep, the first-hit kernel and k_tet_forward run twice).  Every call exact."""
    from dmesh_renderer_amd import _C
    refs = _redo_refs(oracle)
    H, W = TC.REDO["H"], TC.REDO["W"]
    small, big = (refs[s].st.num_rendered for s in sorted(refs))
    assert big > TC.padded(small)
    redo0 = _C.redo_count()
    _C.overflowed()
    for scale in TC.REDO["scales"]:
        ref = refs[scale]
        args = c_args(ref.d, hip_device, tet=True)
        out = _C.render_tets(*args, H, W, 0)
        g = _C.render_tets_backward(*args, ref.gc.to(hip_device), ref.gd.to(hip_device), *out[3:7])
        th.cuda.synchronize()
        ec, ed, R = check_forward(_C, ref, args, out, min_active=0.0)   # (the small scene covers a few tiles)
        eg = check_grads(ref, g, scale)
        print(f"\nscale {scale}: R {R}, longest march {int(ref.st.get('n_contrib').max())}, colour {ec:.2e}, gradients {max(eg):.2e}, "
              f"redos so far {_C.redo_count() - redo0}")
    assert _C.redo_count() >= redo0 + 2, "the refuted guesses must have gone through the redo path"
    assert not _C.overflowed()


def test_tet_async_overflow_is_flagged(oracle, hip_device):
    """An asynchronous tet forward whose lists outgrow the capacity guessed from the default call before it: it cannot redo, so
    it must say so.  (What it is defined to do, dmr_api.hip / dmr_binning.hip / dmr_tet.hip: the scatter drops the entries beyond
    the capacity, k_tet_first_intersect treats a list that ends beyond it as empty, the scan raises the sticky overflow word.)
    The flag is cleared by the read, and a following default call is exact again."""
    from dmesh_renderer_amd import _C
    refs = _redo_refs(oracle)
    H, W = TC.REDO["H"], TC.REDO["W"]
    small, big = (refs[s] for s in sorted(refs))
    assert big.st.num_rendered > TC.padded(small.st.num_rendered)
    sargs, bargs = c_args(small.d, hip_device, tet=True), c_args(big.d, hip_device, tet=True)
    _C.overflowed()
    try:
        out = _C.render_tets(*sargs, H, W, 0)   # default call: leaves the estimate (and the overflow word)
        check_forward(_C, small, sargs, out, min_active=0.0)
        _C.set_async(True)
        assert _C.is_async()
        out = _C.render_tets(*bargs, H, W, 0)   # (never waits: the size is not read back, the capacity is the estimate's)
        th.cuda.synchronize()
        assert _C.overflowed(), "overflow of an asynchronous call must be reported"
        assert not _C.overflowed(), "the flag is cleared by the read"
        assert bool(th.isfinite(out[0]).all())
        _C.set_async(False)
        out = _C.render_tets(*bargs, H, W, 0)   # ... and the default call repairs it
        g = _C.render_tets_backward(*bargs, big.gc.to(hip_device), big.gd.to(hip_device), *out[3:7])
        th.cuda.synchronize()
        check_forward(_C, big, bargs, out, min_active=0.0)
        check_grads(big, g)
        assert not _C.overflowed()
    finally:
        _C.set_async(False)
        _C.overflowed()
