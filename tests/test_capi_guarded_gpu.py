"""Every call path of the C ABI (include/dmesh_renderer_amd.h) through ctypes under a guarded, poisoned allocator
(harness.GuardedCalls): dmr_tri_forward, dmr_tri_backward, dmr_tet_forward and dmr_tet_backward over every DMR_FLAG_* and all
fourteen DMR_BUF_* ids.  Every buffer served through `alloc` and every caller-owned output lies between two 4096-byte guards,
checked after every call; every case runs under both FILLS (scratch 0x00 and outputs 0, scratch 0xA5 and outputs a NaN
pattern) and the two runs are compared; every guarded call of this file goes through checked(), which holds its request log
to the header (check_log) knowing how far dmr_redo_count() grew and, from the per-stage launch counters, whether a tri forward
was a placed one.

What is compared with what:
  a, b  the flag matrices: images, num_rendered and the fragment lists bit for bit those of the same scene through
        dmesh_renderer_amd._C with the same options (the lists unpacked here from the header's text: face | bary | count), the
        gradients -- DMR_BUF_TRI_CAMERA_GRADS, DMR_BUF_TET_GRADS and DMR_BUF_TET_CAMERA_GRADS unpacked by the header's layouts --
        within sum_order_tol(name) of the binding's (rel_err; the matrices' gradients under their own names); outside a band
        every output pixel keeps the pre-fill's bits.  A tet configuration is three forward + backward calls behind a primer
        (the mesh moved off screen: longest march 0, so the next forward has no march sequence): the first backward re-marches,
        the later ones read the sequence (dmr_export "tet_seq").
  c     default flags against the CPU oracle at the project's bars (test_tet_paths_gpu's FWD_TOL, GRAD_TOL, index arrays
        exact), and one opt-in gradient per renderer against its float64 model at grad_cases' bounds.
  d     sizes that grow: the tet REDO pair by default calls (redos under guards) and asynchronously (overflow flagged, finite,
        repaired), a march sequence shorter than the marches taken, and an asynchronous tri backward whose records outgrow the
        capacity the previous default call left.
  f     idle calls (P == 0, F == 0, an empty band): what is requested, what stays untouched, what is zeroed, and what the
        per-stage counters say was launched: nothing in a tri forward with P == 0 / F == 0 and in any idle backward (their
        zeroing is memsets and one untimed fill kernel, which the counters do not see); an empty band's forward does run its
        front end, since it has geometry, and no compositing or march kernel.
One call that looks idle is not, and the header is held: dmr_tet_forward with P == 0 or F == 0 launches, like the reference's,
and "every pixel of the rendered tile rows of all three outputs is written (background / 1 / 0)";
only the fragment buffer is "not at all" requested.  The tri calls and every empty band keep the pre-fill.  And DMR_BUF_WORK,
like DMR_BUF_BINNING, may be requested a second time (larger) by a call that redoes a refuted size guess (header: dmr_alloc_fn):
check_log allows a second request of either only in a call during which dmr_redo_count() grew.
FOUND by test_tri_async_backward_outgrows_its_records: the header promised that such a second request is the larger one; a
placed tri forward redone because one tile outgrew its segment asked for 756 224 and then 536 576 bytes (the exact size, below
the placement's capacity).  The call is right and the sentence was wrong: the header now says so.  check_log holds "larger"
for every other redo, a tri forward's from a plain estimate included: checked() tells a placed forward by its launches (it
scatters more often than it sets faces up), and that test asserts that its forward is one.

MEASURED on the MI355X (every case prints its own figures, pytest -s).  All guards intact, every image, list, index array and
num_rendered exact (tri R 1740 full frame / 1298 in the band, tet 6036 / 4247), under both fills.
  tri matrix (18 cases): gradients against the binding <= 4.7e-07, between the two fills <= 4.5e-07 (the matrices' gradients
    at 1e-5 like the rest; float atomics: the figures move by ~1e-7 from run to run).
  tet matrix (12 cases): (longest march, capacity) per call (24, 0), (24, 36), (24, 36) -- (24, 4) first with the fragment
    flag; gradients against the binding <= 5.1e-07, between the fills <= 4.5e-07.
  against the oracle: tri colour and depth 0, gradients 6.8e-07; tet colour 2.4e-07, depth 3.0e-07, gradients 4.5e-07.
  against float64: tri exact dL_dverts 1.6e-06 (kept 0.939); tet dL_dverts 1.3e-05, dL_dfintense 1.8e-07 (kept 0.968).
  tet REDO: R 16094 / 31703, longest march 50; the big calls ask for the binning buffer twice (7 950 336, then 8 040 192 bytes);
    colour <= 2.4e-07, depth 3.0e-07, gradients <= 6.1e-07.  Asynchronous: capacity 24213 < R 31703, flagged, finite; the default
    call after it 5.3e-07.  Short sequence: opaque marches 1 step, capacity 8 < longest 50, binning buffer 1 426 176 bytes,
    gradients <= 6.5e-07.
  tri asynchronous backward: its forward placed and redone; capacity 11456 of 36352 records (23232 used), 51 of 72 busy tiles
    dropped, the straddling tile among them; gradients against the masked default call <= 3.9e-07, the default call after it
    (redone once) <= 3.2e-07.
  idle: tri P == 0 / F == 0 request and launch nothing in the forward, the camera gradients alone in the backward; the empty
    bands ask for the scratch and the fragment buffer; tet P == 0 asks for 0 bytes of point and face buffer.
The 44 tests together 2.2 - 2.9 s, the slowest 0.4 s.

MUTANTS (scratch builds of the library, nothing of them in the tree; each stray store stays inside the 4096-byte guard; older
tests were run against a mutant only where its stray stores are bounded there too):
  DMR_BUF_BINNING of a tet forward asked for 256 bytes short, kernels unchanged: "the guard behind BINNING was overwritten" in 8
    cases of test_tet_flag_matrix (the calls without the fragment flag) and in test_tet_redo_under_guards.  No older test reaches
    dmr_tet_forward with guards; through the binding the store lands in a neighbouring cached block (not run: unbounded there).
  DMR_BUF_WORK of a tri backward 256 bytes short: "the guard behind WORK" in test_tri_async_backward_outgrows_its_records (the one
    call whose records fill the buffer to its end); the older guarded tests (test_tri_placed_paths_gpu, overflowing pairs) pass.
  DMR_BUF_TET_GRADS 256 bytes short: "the guard behind TET_GRADS" in the 8 cases of test_tet_flag_matrix that own the buffer,
    test_tet_full_grads_match_float64_model and test_tet_idle_calls; tests/test_tet_full_grads_gpu.py passes (the binding hands
    the library its full-size tensor whatever it asks for).
  dL_dfintense of DMR_BUF_TET_GRADS one float early (at 3P - 1): test_tet_full_grads_match_float64_model (dL_dverts 5.5e-03,
    dL_dfintense 1.0); the comparisons with the binding cannot see it (both sides unpack the same buffer); the older
    tests/test_tet_full_grads_gpu.py fails too.
"""
import numpy as np
import pytest
import torch as th

import tet_cases as TC
import test_tet_paths_gpu as TP
from dmesh_renderer_amd import scenes
from grad_cases import FINT_TOL, TET_VERTS_TOL, TRI_VERTS_TOL
from harness import GuardedCalls
from tet_grad_ref import TetGradRef
from tri_grad_ref import TriGradRef
from tri_placed_cases import tile_pixels
from util import BG, c_args, rel_err, sum_order_tol, upstream_grads, with_bg

pytestmark = pytest.mark.gpu

K = 4
FILLS = {"zero": (0x00, 0), "poison": (0xA5, GuardedCalls.NAN_BITS)}   # name: (body fill, the outputs' pre-fill)
TRI = dict(B=2, H=96, W=160)
TET = dict(B=2, H=96, W=176)
BAND = (2, 5)           # tile rows: H = 96 has six, the band starts and ends inside the image
EMPTY_BAND = (6, 6)
TILE = 16
ALL_MATS = 15           # all four mats_transposed bits


def up(n):
    """the header's "every sub-array rounded up to 256" """
    return (n + 255) // 256 * 256


def tri_scene():
    return with_bg(scenes.layered_sheets(3, 9, TRI["B"], TRI["H"], TRI["W"], seed=4), BG)


def tet_scene():
    return with_bg(scenes.kuhn_tets(4, TET["B"], TET["H"], TET["W"], seed=3), BG)


def upstream(B, H, W, alpha):
    """dL/dcolor, dL/ddepth ([B,2,H,W] with alpha: dL/ddepth | dL/dalpha)"""
    gc, gd = upstream_grads(B, H, W)
    if alpha:
        gd = th.cat([gd, th.randn(B, 1, H, W, generator=th.Generator().manual_seed(5))], dim=1)
    return gc, gd


def bary_grads(B, H, W):
    return th.randn(B, K, 2, H, W, generator=th.Generator().manual_seed(6))


# ---- the header's layouts ------------------------------------------------------------------------------------------------------
def unpack_fragments(body, B, H, W):
    """DMR_BUF_*_FRAGMENTS: face int32 [B,K,H,W] | bary fp32 [B,K,2,H,W] | count int32 [B,H,W], back to back."""
    n = B * H * W
    assert body.numel() == 4 * n * (3 * K + 1)
    words = body.view(th.int32)
    return {"face": words[:K * n].view(B, K, H, W), "bary": words[K * n:3 * K * n].view(th.float32).view(B, K, 2, H, W),
            "count": words[3 * K * n:].view(B, H, W)}


def unpack_mats(body, B, names):
    """fp32 [B][16 per name], each matrix in the contract layout m[4*col+row] whatever mats_transposed says -> {name: [B,4,4]},
    element [b, col, row]: what the binding returns as the gradient of the transposed tensor it was given."""
    m = body.view(th.float32).view(B, len(names), 16)
    out = {}
    for i, name in enumerate(names):
        g = th.empty(B, 4, 4, device=body.device)
        for col in range(4):
            for row in range(4):
                g[:, col, row] = m[:, i, 4 * col + row]
        out[name] = g
    return out


def unpack_tet_grads(body, P, B, F):
    """DMR_BUF_TET_GRADS = [dL_dverts [P,3] | dL_dfintense [B,F]]"""
    w = body.view(th.float32)
    assert w.numel() == 3 * P + B * F
    return {"verts": w[:3 * P].view(P, 3), "faces_intense": w[3 * P:].view(B, F)}


# ---- the request contract (f) --------------------------------------------------------------------------------------------------
def check_log(capi, kind, log, flags, B, P, F, H, W, rows, redone, R=None, placed=False):
    """One call's requests against the header: which ids (none that the header does not attach to the call and its flags, every
    one it does), each once -- a second, larger request only of the speculatively sized buffer of a call that redid a refuted
    guess; placed: a tri forward binned into placed segments (checked() tells by its launches), whose second request may be the
    smaller --, and the byte counts the header states exactly."""
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    r0, r1 = rows if rows != (0, 0) else (0, gy)
    r0 = max(0, min(gy, r0)); r1 = max(r0, min(gy, r1))
    geometry, band = P > 0 and F > 0, r1 > r0
    nt, npix = B * gx * gy, B * W * H
    want, exact, optional, twice = set(), {}, set(), None
    if kind in ("tri_forward", "tet_forward"):
        frag_flag, frag_id = ((capi.FLAG_TRI_FRAGMENTS, capi.BUF_TRI_FRAGMENTS) if kind == "tri_forward" else
                              (capi.FLAG_TET_FRAGMENTS, capi.BUF_TET_FRAGMENTS))
        if geometry or kind == "tet_forward":
            want |= {capi.BUF_POINT, capi.BUF_FACE, capi.BUF_IMAGE}
            optional.add(capi.BUF_BINNING)   # (every call asks, a call without entries or sequence for 0 bytes)
            twice = capi.BUF_BINNING
        if (flags & frag_flag) and geometry:
            want.add(frag_id)
            exact[frag_id] = 4 * npix * (3 * K + 1)
    elif kind == "tri_backward":
        idle = not geometry or not band or R <= 0
        if flags & capi.FLAG_TRI_CAMERA_GRADS:
            want.add(capi.BUF_TRI_CAMERA_GRADS)
            exact[capi.BUF_TRI_CAMERA_GRADS] = 128 * B
        if not idle:
            want.add(capi.BUF_WORK)
            twice = capi.BUF_WORK
            if flags & capi.FLAG_TRI_FRAGMENT_GRADS:
                want |= {capi.BUF_TRI_FRAGMENT_FACES, capi.BUF_TRI_FRAGMENT_BARY_GRADS}
                exact[capi.BUF_TRI_FRAGMENT_FACES], exact[capi.BUF_TRI_FRAGMENT_BARY_GRADS] = 4 * K * npix, 8 * K * npix
    else:
        assert kind == "tet_backward"
        camera = bool(flags & capi.FLAG_TET_CAMERA_GRADS)
        full = camera or bool(flags & (capi.FLAG_TET_FULL_GRADS | capi.FLAG_TET_FRAGMENT_GRADS))
        if full and 3 * P + B * F > 0:
            want.add(capi.BUF_TET_GRADS)
            exact[capi.BUF_TET_GRADS] = 4 * (3 * P + B * F)
        if camera:
            want.add(capi.BUF_TET_CAMERA_GRADS)
            exact[capi.BUF_TET_CAMERA_GRADS] = 256 * B
            if geometry and band:
                want.add(capi.BUF_WORK)
                exact[capi.BUF_WORK] = 256 * gx * (r1 - r0) * B   # "256 per tile of the call's band"
        if (flags & capi.FLAG_TET_FRAGMENT_GRADS) and geometry and band:
            want |= {capi.BUF_TET_FRAGMENT_FACES, capi.BUF_TET_FRAGMENT_BARY_GRADS}
            exact[capi.BUF_TET_FRAGMENT_FACES], exact[capi.BUF_TET_FRAGMENT_BARY_GRADS] = 4 * K * npix, 8 * K * npix
    names = lambda ids: sorted(capi.BUF_NAMES[i] for i in ids)
    asked = [w for w, _ in log]
    assert set(asked) <= want | optional, (kind, "requested beyond the header:", names(set(asked) - want - optional))
    assert want <= set(asked), (kind, "not requested:", names(want - set(asked)))
    for w in set(asked):
        sizes = [n for i, n in log if i == w]
        if len(sizes) > 1:
            assert w == twice and redone > 0 and len(sizes) == 2, (kind, capi.BUF_NAMES[w], sizes, redone)
            # the larger: sized() redoes an estimate only when the exact size exceeds it.  But a PLACED tri forward is redone when
            # ONE tile outgrew its segment, and the exact size it then asks for may be below the placement's capacity (header,
            # dmr_alloc_fn)
            assert sizes[1] > sizes[0] or placed, (kind, capi.BUF_NAMES[w], sizes)
        if w in exact:
            assert sizes == [exact[w]], (kind, capi.BUF_NAMES[w], sizes, exact[w])
    size = dict(log)
    if kind.endswith("forward") and capi.BUF_POINT in size:   # the footprints the header gives as sums: never less
        assert size[capi.BUF_POINT] >= 16 * B * P and size[capi.BUF_FACE] >= 16 * B * F and size[capi.BUF_IMAGE] >= 40 * nt + 12 * npix
    if kind == "tri_backward" and capi.BUF_WORK in size:
        assert size[capi.BUF_WORK] >= 32 * B * P + 8 * B * F + 8192 * nt


def launches(fn):
    """fn() with the per-stage profile on -> (fn's result, {stage name: launches})"""
    from dmesh_renderer_amd import _C
    th.cuda.synchronize()
    _C.profile_collect()
    _C.profile_enable(0xfff)
    try:
        r = fn()
        th.cuda.synchronize()
        _, n = _C.profile_collect()
    finally:
        _C.profile_enable(0)
    return r, {_C.stage_name(i): int(k) for i, k in enumerate(n)}


def checked(calls, kind, d, H, W, flags, rows, fn, R=None):
    """fn(): ONE guarded call of `kind`.  Its request log against the header (check_log), with what the test can know of the
    call from outside: how far dmr_redo_count() grew and, for a tri forward, whether it binned into placed segments -- a placed
    call scatters (k_bin_faces, timed as k_scatter_faces) without a face set-up of its own; redone, it adds the exact path's one
    set-up and one scatter, where a refuted estimate runs the set-up twice.  -> (fn's result, {stage name: launches})"""
    B, P, F = d["mv_mats"].shape[0], d["verts"].shape[0], d["faces"].shape[0]
    redo0 = calls.lib.dmr_redo_count()
    r, n = launches(fn)
    placed = kind == "tri_forward" and n["k_scatter_faces"] > n["k_setup_faces"]
    check_log(calls.capi, kind, r.log, flags, B, P, F, H, W, rows, calls.lib.dmr_redo_count() - redo0, R=R, placed=placed)
    r.placed = placed
    return r, n


# ---- one guarded step ----------------------------------------------------------------------------------------------------------
TRI_GRADS = ("verts", "verts_color", "faces_opacity", "verts_depth", "faces_intense")
TET_GRADS = ("verts_color", "faces_opacity")


def tri_step(calls, d, H, W, flags, rows=(0, 0), mats=0, gbary=None):
    """dmr_tri_forward + dmr_tri_backward, logs checked -> {"R", "images": {..}, "grads": {..}, "fwd", "bwd"}"""
    capi, lib = calls.capi, calls.lib
    B, P, F = d["mv_mats"].shape[0], d["verts"].shape[0], d["faces"].shape[0]
    alpha = bool(flags & capi.FLAG_ALPHA)
    gc, gd = upstream(B, H, W, alpha)
    f, _ = checked(calls, "tri_forward", d, H, W, flags, rows, lambda: calls.tri_forward(d, H, W, flags, rows, mats))
    images = {"color": f.color, "depth": f.depth}
    if f.fragments is not None:
        images.update(unpack_fragments(f.fragments, B, H, W))
    if flags & capi.FLAG_TRI_FRAGMENT_GRADS:   # the inputs: this forward's own faces (outside a band: the pre-fill, no face of the mesh)
        calls.inputs = {capi.BUF_TRI_FRAGMENT_FACES: images["face"].clone(), capi.BUF_TRI_FRAGMENT_BARY_GRADS: gbary.to(calls.dev)}
    b, _ = checked(calls, "tri_backward", d, H, W, flags, rows, lambda: calls.tri_backward(d, H, W, flags, f.R, gc, gd, rows, mats), R=f.R)
    grads = dict(zip(TRI_GRADS, b.grads))
    if b.camera is not None:
        grads.update(unpack_mats(b.camera, B, ("inv_mv", "inv_proj")))
    return {"R": f.R, "images": images, "grads": grads, "fwd": f, "bwd": b}


def tet_step(calls, d, H, W, flags, rows=(0, 0), mats=0, gbary=None, seed=0, fwd_flags=None):
    """dmr_tet_forward + dmr_tet_backward, logs checked -> {"R", "images", "grads", "seq": (longest march, capacity), "fwd", "bwd"}"""
    from dmesh_renderer_amd import _C
    capi, lib = calls.capi, calls.lib
    B, P, F = d["mv_mats"].shape[0], d["verts"].shape[0], d["faces"].shape[0]
    alpha = bool(flags & capi.FLAG_ALPHA)
    gc, gd = upstream(B, H, W, alpha)
    fflags = flags if fwd_flags is None else fwd_flags
    f, _ = checked(calls, "tet_forward", d, H, W, fflags, rows, lambda: calls.tet_forward(d, H, W, fflags, rows, mats, seed))
    images = {"color": f.color, "depth": f.depth, "active": f.active}
    if f.fragments is not None:
        images.update(unpack_fragments(f.fragments, B, H, W))
    if flags & capi.FLAG_TET_FRAGMENT_GRADS:
        calls.inputs = {capi.BUF_TET_FRAGMENT_FACES: images["face"].clone(), capi.BUF_TET_FRAGMENT_BARY_GRADS: gbary.to(calls.dev)}
    b, _ = checked(calls, "tet_backward", d, H, W, flags, rows, lambda: calls.tet_backward(d, H, W, flags, gc, gd, rows, mats, seed))
    grads = dict(zip(TET_GRADS, b.grads))
    if b.full is not None:
        grads.update(unpack_tet_grads(b.full, P, B, F))
    if b.camera is not None:
        grads.update(unpack_mats(b.camera, B, ("inv_mv", "inv_proj", "mv", "proj")))
    seq = None
    if P > 0 and F > 0:
        bufs = [calls.buffers[w] for w in range(4)]
        seq = tuple(int(x) for x in _C.export("tet_seq", f.args, True, 0, bufs, H, W, th.int32).cpu().numpy().view(np.uint32)[:2])
    return {"R": f.R, "images": images, "grads": grads, "seq": seq, "fwd": f, "bwd": b}


# ---- comparisons ---------------------------------------------------------------------------------------------------------------
def band_px(H, rows):
    gy = (H + TILE - 1) // TILE
    r0, r1 = rows if rows != (0, 0) else (0, gy)
    return TILE * min(r0, gy), min(H, TILE * min(r1, gy))


def bits(t):
    return t.contiguous().view(th.int32) if t.dtype == th.float32 else t


def same_images(got, want, H, rows, what):
    """bit for bit on the rendered rows (H is the last dimension but one of every image and list)"""
    y0, y1 = band_px(H, rows)
    assert sorted(got) == sorted(want), (what, sorted(got), sorted(want))
    for k in got:
        a, b = bits(got[k])[..., y0:y1, :], bits(want[k].to(got[k].device))[..., y0:y1, :]
        assert a.shape == b.shape and th.equal(a, b), (what, k, int((a != b).sum()))


def untouched_outside(calls, images, H, rows, what):
    """outside the band every output still holds the pre-fill's exact bits"""
    y0, y1 = band_px(H, rows)
    for k, t in images.items():
        pre = bits(calls.prefill(t))
        assert th.equal(bits(t)[..., :y0, :], pre[..., :y0, :]) and th.equal(bits(t)[..., y1:, :], pre[..., y1:, :]), (what, k)


def grad_tol(name):
    return sum_order_tol(name)


def close_grads(got, want, what):
    """every gradient finite (a NaN of the pre-fill left anywhere fails here) and within grad_tol(name) -> the largest error"""
    assert sorted(got) == sorted(want), (what, sorted(got), sorted(want))
    worst = 0.0
    for k in got:
        a, b = got[k].cpu().numpy(), want[k].cpu().numpy()
        assert a.shape == b.shape and np.isfinite(a).all(), (what, k)
        e = rel_err(a, b)
        assert e <= grad_tol(k), (what, k, e)
        worst = max(worst, e)
    return worst


# ---- a, e, f: the tri flag matrix ----------------------------------------------------------------------------------------------
def tri_flag_sets(capi):
    frag = capi.fragments_flags(K) | capi.FLAG_TRI_FRAGMENT_GRADS
    every = capi.FLAG_TRI_EXACT_GRADS | capi.FLAG_TRI_CAMERA_GRADS | capi.FLAG_ALPHA | frag
    return {"default": 0, "exact": capi.FLAG_TRI_EXACT_GRADS, "camera": capi.FLAG_TRI_CAMERA_GRADS, "alpha": capi.FLAG_ALPHA,
            "fragments": frag, "all": every}


_binding = {}


def tri_binding(dev, capi, name, rows):
    """The same scene through dmesh_renderer_amd._C with the same options, once per (flag set, band)."""
    from dmesh_renderer_amd import _C
    if ("tri", name, rows) not in _binding:
        flags = tri_flag_sets(capi)[name]
        d, (B, H, W) = tri_scene(), (TRI["B"], TRI["H"], TRI["W"])
        alpha, frag = bool(flags & capi.FLAG_ALPHA), bool(flags & capi.FLAG_TRI_FRAGMENTS)
        args = c_args(d, dev)
        gc, gd = (x.to(dev) for x in upstream(B, H, W, alpha))
        out = _C.render_tris(*args, H, W, rows=rows, alpha=alpha, fragments=K if frag else 0)
        g = _C.render_tris_backward(*args, gc, gd, out[0], *out[3:7], rows=rows, exact_grads=bool(flags & capi.FLAG_TRI_EXACT_GRADS),
                                    camera_grads=bool(flags & capi.FLAG_TRI_CAMERA_GRADS), alpha=alpha,
                                    fragment_grads=(out[7], bary_grads(B, H, W).to(dev)) if frag else None)
        th.cuda.synchronize()
        images = {"color": out[1], "depth": out[2]}
        if frag:
            images.update(face=out[7], bary=out[8], count=out[9])
        _binding["tri", name, rows] = {"R": out[0], "images": images, "grads": dict(zip(TRI_GRADS + ("inv_mv", "inv_proj"), g))}
    return _binding["tri", name, rows]


@pytest.mark.parametrize("mode", ["full", "band", "transposed"])
@pytest.mark.parametrize("name", ["default", "exact", "camera", "alpha", "fragments", "all"])
def test_tri_flag_matrix(hip_device, name, mode):
    import capi_ctypes as capi
    flags = tri_flag_sets(capi)[name]
    rows, mats = (BAND if mode == "band" else (0, 0)), (ALL_MATS if mode == "transposed" else 0)
    d, H, W = tri_scene(), TRI["H"], TRI["W"]
    ref = tri_binding(hip_device, capi, name, rows)
    runs, worst = {}, 0.0
    for fill, (body, out_bits) in FILLS.items():
        calls = GuardedCalls(hip_device, body, out_bits)
        r = runs[fill] = tri_step(calls, d, H, W, flags, rows, mats, gbary=bary_grads(TRI["B"], H, W))
        what = (name, mode, fill)
        assert r["R"] == ref["R"] > 0, what
        same_images(r["images"], ref["images"], H, rows, what)
        untouched_outside(calls, r["images"], H, rows, what)
        worst = max(worst, close_grads(r["grads"], ref["grads"], what))
        assert float(r["grads"]["verts"].abs().max()) > 0
    a, b = runs["zero"], runs["poison"]
    assert a["R"] == b["R"]
    same_images(a["images"], b["images"], H, rows, (name, mode, "zero vs poison"))
    between = close_grads(a["grads"], b["grads"], (name, mode, "zero vs poison"))
    print(f"\ntri {name} {mode}: R {a['R']}, requests {[(capi.BUF_NAMES[w], n) for w, n in a['fwd'].log + a['bwd'].log]}; gradients vs the "
          f"binding {worst:.2e}, between the fills {between:.2e}")


# ---- b, e, f: the tet flag matrix ----------------------------------------------------------------------------------------------
def tet_flag_sets(capi):
    frag = capi.tet_fragments_flags(K) | capi.FLAG_TET_FRAGMENT_GRADS
    every = capi.FLAG_TET_FULL_GRADS | capi.FLAG_TET_CAMERA_GRADS | capi.FLAG_ALPHA | frag
    return {"default": 0, "full": capi.FLAG_TET_FULL_GRADS, "camera": capi.FLAG_TET_CAMERA_GRADS, "alpha": capi.FLAG_ALPHA,
            "fragments": frag, "all": every}


def tet_binding(dev, capi, name, rows):
    from dmesh_renderer_amd import _C
    if ("tet", name, rows) not in _binding:
        flags = tet_flag_sets(capi)[name]
        d, (B, H, W) = tet_scene(), (TET["B"], TET["H"], TET["W"])
        alpha, frag = bool(flags & capi.FLAG_ALPHA), bool(flags & capi.FLAG_TET_FRAGMENTS)
        camera = bool(flags & capi.FLAG_TET_CAMERA_GRADS)
        full = camera or frag or bool(flags & capi.FLAG_TET_FULL_GRADS)
        args = c_args(d, dev, tet=True)
        gc, gd = (x.to(dev) for x in upstream(B, H, W, alpha))
        out = _C.render_tets(*args, H, W, 0, rows=rows, alpha=alpha, fragments=K if frag else 0)
        g = _C.render_tets_backward(*args, gc, gd, *out[3:7], rows=rows, full_grads=full, camera_grads=camera, alpha=alpha,
                                    fragment_grads=(out[7], bary_grads(B, H, W).to(dev)) if frag else None)
        th.cuda.synchronize()
        ranges = _C.export("ranges", args, True, 0, out[3:7], H, W, th.int32).cpu().numpy().view(np.uint32)
        images = {"color": out[0], "depth": out[1], "active": out[2]}
        if frag:
            images.update(face=out[7], bary=out[8], count=out[9])
        order = ("verts", "verts_color", "faces_opacity", "faces_intense", "inv_mv", "inv_proj", "mv", "proj") if full else TET_GRADS
        _binding["tet", name, rows] = {"R": int(ranges.max()), "images": images, "grads": dict(zip(order, g))}
    return _binding["tet", name, rows]


def off_screen(d):
    """The mesh far to the side of every camera's frustum: same shapes (the same view configuration and mesh-size bucket), no
    face on screen, no march -- the backward of such a call leaves a longest march of 0 for the next forward's estimate."""
    return dict(d, verts=d["verts"] + th.tensor([60.0, 0.0, 0.0]))


def estimate(longest):
    """dmr_api.hip, march_estimate: the steps per pixel the next forward's sequence has room for"""
    return (longest + longest // 4 + 4 + 3) // 4 * 4 if longest else 0


@pytest.mark.parametrize("mode", ["full", "band"])
@pytest.mark.parametrize("name", ["default", "full", "camera", "alpha", "fragments", "all"])
def test_tet_flag_matrix(hip_device, name, mode):
    import capi_ctypes as capi
    flags = tet_flag_sets(capi)[name]
    rows = BAND if mode == "band" else (0, 0)
    d, H, W = tet_scene(), TET["H"], TET["W"]
    ref = tet_binding(hip_device, capi, name, rows)
    k_steps = (K + 3) // 4 * 4 if flags & capi.FLAG_TET_FRAGMENTS else 0
    runs, worst, seqs = {}, 0.0, []
    for fill, (body, out_bits) in FILLS.items():
        calls = GuardedCalls(hip_device, body, out_bits)
        primer = tet_step(calls, off_screen(d), H, W, 0, rows)
        assert primer["R"] == 0 and primer["seq"][0] == 0 and float(primer["images"]["active"][:, band_px(H, rows)[0]].abs().max()) == 0.0
        runs[fill] = []
        for call in range(3):
            r = tet_step(calls, d, H, W, flags, rows, gbary=bary_grads(TET["B"], H, W))
            runs[fill].append(r)
            what = (name, mode, fill, call)
            longest, cap = r["seq"]
            if call == 0:   # no estimate: no sequence beyond the fragments' K steps, the backward re-marches
                assert cap == k_steps and longest > cap, (what, longest, cap)
            else:           # the sequence is complete: k_tet_backward_seq did the work
                assert 0 < longest <= cap == max(k_steps, estimate(longest)), (what, longest, cap)
            assert r["R"] == ref["R"] > 0, what
            same_images(r["images"], ref["images"], H, rows, what)
            untouched_outside(calls, r["images"], H, rows, what)
            worst = max(worst, close_grads(r["grads"], ref["grads"], what))
            assert float(r["grads"]["faces_opacity"].abs().max()) > 0
        seqs.append([r["seq"] for r in runs[fill]])
    between = 0.0
    for a, b in zip(runs["zero"], runs["poison"]):
        assert a["R"] == b["R"] and a["seq"] == b["seq"]
        same_images(a["images"], b["images"], H, rows, (name, mode, "zero vs poison"))
        between = max(between, close_grads(a["grads"], b["grads"], (name, mode, "zero vs poison")))
    a = runs["zero"][1]
    print(f"\ntet {name} {mode}: R {a['R']}, (longest march, capacity) per call {seqs[0]}, requests "
          f"{[(capi.BUF_NAMES[w], n) for w, n in a['fwd'].log + a['bwd'].log]}; gradients vs the binding {worst:.2e}, between the fills {between:.2e}")


# ---- c: against the references directly ----------------------------------------------------------------------------------------
def test_tri_default_call_is_the_oracles(oracle, hip_device):
    from dmesh_renderer_amd import _C
    import capi_ctypes as capi
    d, B, H, W = tri_scene(), TRI["B"], TRI["H"], TRI["W"]
    sc = oracle.scene_from_module_inputs(d, H, W)
    oc, od, ost = oracle.tri_forward(sc)
    gc, gd = upstream(B, H, W, False)
    og = oracle.tri_backward(sc, ost, gc.numpy(), gd.numpy())
    for fill, (body, out_bits) in FILLS.items():
        calls = GuardedCalls(hip_device, body, out_bits)
        r = tri_step(calls, d, H, W, 0)
        assert r["R"] == ost.num_rendered
        bufs = [calls.buffers[w] for w in range(4)]
        ex = lambda n: _C.export(n, r["fwd"].args, False, r["R"], bufs, H, W, th.int32).cpu().numpy().view(np.uint32)
        np.testing.assert_array_equal(ex("ranges"), ost.get("ranges"))
        np.testing.assert_array_equal(ex("face_list"), ost.get("values"))
        np.testing.assert_array_equal(ex("n_contrib"), ost.get("n_contrib"))
        ec = float(np.abs(r["images"]["color"].cpu().numpy() - oc).max())
        ed = float(np.abs(r["images"]["depth"].cpu().numpy() - od).max())
        errs = {k: rel_err(r["grads"][k].cpu().numpy(), og[k]) for k in TRI_GRADS}
        print(f"\ntri vs the oracle ({fill}): R {r['R']}, colour {ec:.2e}, depth {ed:.2e}, gradients {max(errs.values()):.2e}")
        assert ec <= TP.FWD_TOL and ed <= TP.FWD_TOL, (ec, ed)
        assert max(errs.values()) <= TP.GRAD_TOL, errs


_tet_refs = {}


def tet_ref(oracle, key):
    """The oracle's forward and gradients: "matrix" the tet matrix scene, a float the REDO scene of that scale; once each."""
    if key not in _tet_refs:
        if key == "matrix":
            _tet_refs[key] = TC.Ref(oracle, tet_scene(), TET["B"], TET["H"], TET["W"])
        else:
            _tet_refs[key] = TC.Ref(oracle, with_bg(TC.redo_scene(key), BG), TC.REDO["B"], TC.REDO["H"], TC.REDO["W"])
    return _tet_refs[key]


def check_tet_against_oracle(calls, ref, r, what, min_active=0.2):
    """test_tet_paths_gpu's checks (index arrays and topology exact, images FWD_TOL, gradients GRAD_TOL) on a guarded step"""
    from dmesh_renderer_amd import _C
    out = (r["images"]["color"], r["images"]["depth"], r["images"]["active"]) + tuple(calls.buffers[w] for w in range(4))
    ec, ed, R = TP.check_forward(_C, ref, r["fwd"].args, out, min_active=min_active)
    assert R == r["R"]
    eg = TP.check_grads(ref, [r["grads"][k] for k in TET_GRADS], what)
    return ec, ed, max(eg)


def test_tet_default_call_is_the_oracles(oracle, hip_device):
    ref = tet_ref(oracle, "matrix")
    for fill, (body, out_bits) in FILLS.items():
        calls = GuardedCalls(hip_device, body, out_bits)
        for call in range(2):   # the re-marching backward or the sequence's, as the estimate has it
            r = tet_step(calls, ref.d, ref.H, ref.W, 0)
            ec, ed, eg = check_tet_against_oracle(calls, ref, r, (fill, call))
            print(f"\ntet vs the oracle ({fill}, call {call}): R {r['R']}, (longest, capacity) {r['seq']}, colour {ec:.2e}, depth {ed:.2e}, "
                  f"gradients {eg:.2e}")


def test_tri_exact_grads_match_float64_model(oracle, hip_device):
    """DMR_FLAG_TRI_EXACT_GRADS through the C ABI against tests/tri_grad_ref.py, at test_tri_exact_grads_gpu's bound."""
    import capi_ctypes as capi
    d, B, H, W = tri_scene(), TRI["B"], TRI["H"], TRI["W"]
    _, _, ost = oracle.tri_forward(oracle.scene_from_module_inputs(d, H, W))
    model = TriGradRef(d, H, W, ost)
    assert model.kept_fraction >= 0.8, model.kept_fraction
    gc, gd = upstream_grads(B, H, W)
    m = model.mask()
    gc, gd = gc * m, gd * m
    rg, _, _ = model.grads(gc, gd)
    for fill, (body, out_bits) in FILLS.items():
        calls = GuardedCalls(hip_device, body, out_bits)
        flags = capi.FLAG_TRI_EXACT_GRADS
        f, _ = checked(calls, "tri_forward", d, H, W, flags, (0, 0), lambda: calls.tri_forward(d, H, W, flags))
        b, _ = checked(calls, "tri_backward", d, H, W, flags, (0, 0), lambda: calls.tri_backward(d, H, W, flags, f.R, gc, gd), R=f.R)
        ev = rel_err(b.grads[0].cpu().numpy(), rg["verts"])
        print(f"\ntri exact dL_dverts vs float64 ({fill}): {ev:.2e} (kept {model.kept_fraction:.3f})")
        assert ev <= TRI_VERTS_TOL, ev


def test_tet_full_grads_match_float64_model(oracle, hip_device):
    """DMR_FLAG_TET_FULL_GRADS through the C ABI, DMR_BUF_TET_GRADS unpacked by the header, against tests/tet_grad_ref.py at
    test_tet_full_grads_gpu's bounds."""
    import capi_ctypes as capi
    d, B, H, W = tet_scene(), TET["B"], TET["H"], TET["W"]
    ost = tet_ref(oracle, "matrix").st
    model = TetGradRef(d, H, W, ost)
    assert model.kept_fraction >= 0.8, model.kept_fraction
    gc, gd = upstream_grads(B, H, W)
    m = model.mask()
    gc, gd = gc * m, gd * m
    rg, _, _ = model.grads(gc, gd)
    P, F = d["verts"].shape[0], d["faces"].shape[0]
    for fill, (body, out_bits) in FILLS.items():
        calls = GuardedCalls(hip_device, body, out_bits)
        flags = capi.FLAG_TET_FULL_GRADS
        checked(calls, "tet_forward", d, H, W, flags, (0, 0), lambda: calls.tet_forward(d, H, W, flags))
        b, _ = checked(calls, "tet_backward", d, H, W, flags, (0, 0), lambda: calls.tet_backward(d, H, W, flags, gc, gd))
        g = unpack_tet_grads(b.full, P, B, F)
        ev, ei = rel_err(g["verts"].cpu().numpy(), rg["verts"]), rel_err(g["faces_intense"].cpu().numpy(), rg["faces_intense"])
        print(f"\ntet full dL_dverts {ev:.2e}, dL_dfintense {ei:.2e} vs float64 ({fill}; kept {model.kept_fraction:.3f})")
        assert ev <= TET_VERTS_TOL and ei <= FINT_TOL, (ev, ei)


# ---- d: sizes that grow, under guards ------------------------------------------------------------------------------------------
def test_tet_redo_under_guards(oracle, hip_device):
    """The REDO scales small -> big -> small -> big by default calls: the big calls refute the small ones' guess and are redone
    (DMR_BUF_BINNING requested a second time, larger: both buffers' guards are checked); every call the oracle's."""
    import capi_ctypes as capi
    H, W = TC.REDO["H"], TC.REDO["W"]
    runs = {}
    for fill, (body, out_bits) in FILLS.items():
        calls = GuardedCalls(hip_device, body, out_bits)
        calls.lib.dmr_overflowed(-1, 1)
        redo0 = calls.lib.dmr_redo_count()
        runs[fill] = []
        for scale in TC.REDO["scales"]:
            ref = tet_ref(oracle, scale)
            r = tet_step(calls, ref.d, H, W, 0)
            ec, ed, eg = check_tet_against_oracle(calls, ref, r, (fill, scale), min_active=0.0)
            twice = [n for w, n in r["fwd"].log if w == capi.BUF_BINNING]
            print(f"\nscale {scale} ({fill}): R {r['R']}, (longest, capacity) {r['seq']}, binning requests {twice}, colour {ec:.2e}, "
                  f"depth {ed:.2e}, gradients {eg:.2e}")
            runs[fill].append(r)
        assert calls.lib.dmr_redo_count() >= redo0 + 2, "the refuted guesses must have gone through the redo path"
        assert [len([1 for w, _ in r["fwd"].log if w == capi.BUF_BINNING]) for r in runs[fill]][1::2] == [2, 2]
        assert not calls.lib.dmr_overflowed(-1, 1)
    for a, b in zip(runs["zero"], runs["poison"]):
        assert a["R"] == b["R"]
        same_images(a["images"], b["images"], H, (0, 0), "redo, zero vs poison")
        close_grads(a["grads"], b["grads"], "redo, zero vs poison")


def test_tet_async_overflow_under_guards(oracle, hip_device):
    """Small by default, then big with DMR_FLAG_ASYNC: it cannot redo -- guards intact, dmr_overflowed raised, every pixel finite;
    the following default call is exact."""
    import capi_ctypes as capi
    H, W = TC.REDO["H"], TC.REDO["W"]
    small, big = (tet_ref(oracle, s) for s in sorted(set(TC.REDO["scales"])))
    assert big.st.num_rendered > TC.padded(small.st.num_rendered)
    runs = {}
    for fill, (body, out_bits) in FILLS.items():
        calls = GuardedCalls(hip_device, body, out_bits)
        lib = calls.lib
        lib.dmr_overflowed(-1, 1)
        r = tet_step(calls, small.d, H, W, 0)
        check_tet_against_oracle(calls, small, r, (fill, "small"), min_active=0.0)
        a = tet_step(calls, big.d, H, W, capi.FLAG_ASYNC)
        assert lib.dmr_overflowed(-1, 1), "overflow of an asynchronous call must be reported"
        assert not lib.dmr_overflowed(-1, 1), "the flag is cleared by the read"
        # an asynchronous call returns the capacity it used: the small call's R padded (to a unit: the estimate is kept as a ratio)
        assert abs(a["R"] - TC.padded(small.st.num_rendered)) <= 2 and a["R"] < big.st.num_rendered, a["R"]
        for k, t in list(a["images"].items()) + list(a["grads"].items()):
            assert bool(th.isfinite(t).all()), (fill, k)
        r = tet_step(calls, big.d, H, W, 0)
        ec, ed, eg = check_tet_against_oracle(calls, big, r, (fill, "big"), min_active=0.0)
        assert not lib.dmr_overflowed(-1, 1)
        print(f"\nasync overflow ({fill}): capacity {a['R']} < R {r['R']}; the default call after it: colour {ec:.2e}, depth {ed:.2e}, gradients {eg:.2e}")
        runs[fill] = (a, r)
    for a, b in zip(runs["zero"], runs["poison"]):
        assert a["R"] == b["R"]
        same_images(a["images"], b["images"], H, (0, 0), "async, zero vs poison")
        close_grads(a["grads"], b["grads"], "async, zero vs poison")


def test_tet_short_march_sequence_under_guards(oracle, hip_device):
    """The call whose march sequence is shorter than the marches now taken: after a step of the same mesh with every face opaque
    (marches of a step or two) the big scene's forward has room for fewer steps than its rays take -- the march must stop
    storing at the capacity (the sequence is the tail of the binning buffer: its back guard), the backward must see that the
    sequence is incomplete and re-march: the oracle's gradients."""
    H, W = TC.REDO["H"], TC.REDO["W"]
    big = tet_ref(oracle, max(TC.REDO["scales"]))
    opaque = dict(big.d, faces_opacity=th.ones_like(big.d["faces_opacity"]))
    runs = {}
    for fill, (body, out_bits) in FILLS.items():
        calls = GuardedCalls(hip_device, body, out_bits)
        calls.lib.dmr_overflowed(-1, 1)
        p = tet_step(calls, opaque, H, W, 0)
        short = p["seq"][0]
        r = tet_step(calls, big.d, H, W, 0)
        longest, cap = r["seq"]
        assert 0 < cap == estimate(short) < longest, (short, longest, cap)
        sizes = dict(r["fwd"].log)
        ec, ed, eg = check_tet_against_oracle(calls, big, r, fill, min_active=0.0)
        print(f"\nshort sequence ({fill}): opaque marches {short} steps, capacity {cap}, longest march {longest}; binning buffer "
              f"{sizes[calls.capi.BUF_BINNING]} bytes; colour {ec:.2e}, depth {ed:.2e}, gradients {eg:.2e}")
        runs[fill] = r
    same_images(runs["zero"]["images"], runs["poison"]["images"], H, (0, 0), "short sequence, zero vs poison")
    close_grads(runs["zero"]["grads"], runs["poison"]["grads"], "short sequence, zero vs poison")


def test_tri_async_backward_outgrows_its_records(hip_device):
    """An asynchronous tri backward whose blended pairs exceed the record capacity the previous default call left (the matrix scene
    shrunk to 0.3 of its width and height, then at full size; the forwards are default calls, so the lists are exact).

    What the call is defined to do (dmr_api.hip, dmr_tri.hip): the capacity is the estimate's; the tiles' record regions lie in
    tile order, tile t's at the sum of record_bound(tile_hits, list length) of the tiles before it; k_tri_backward_pix stores no
    record at or beyond the capacity and publishes the total, which raises the sticky overflow word; k_tri_backward_hits drops
    every tile whose USED records, in whole blocks of 256, do not end inside the capacity ("the results are thrown away") and
    k_tri_unpack writes all five outputs.  A tile's used records are its blended pairs with every face's run padded to a multiple
    of 4 (HIT_GROUP): formed here from the binding's fragment lists of the same scene (K = 32, no pixel deeper; their sums per
    tile are the forward's tile_hits, exactly).  So the dropped tiles are known, the one that straddles the capacity included,
    and the gradients are the default call's with the upstream gradients zeroed on them (the backward is linear in those).  The
    default call after it redoes once (DMR_BUF_WORK a second time, larger) and is the binding's."""
    from dmesh_renderer_amd import _C
    import capi_ctypes as capi
    B, H, W = TRI["B"], TRI["H"], TRI["W"]
    big = tri_scene()
    small = dict(big, verts=big["verts"] * th.tensor([0.3, 0.3, 1.0]))
    P, F = big["verts"].shape[0], big["faces"].shape[0]
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    nt = B * gx * gy
    args = c_args(big, hip_device)
    gc, gd = upstream(B, H, W, False)
    out = _C.render_tris(*args, H, W, fragments=32)
    face, count = out[7].cpu().numpy(), out[9].cpu().numpy()
    assert int(count.max()) <= 32, "every blended pair is stored"
    vb, vk, vy, vx = np.nonzero(face >= 0)
    tile_of = (vb * gy + vy // TILE) * gx + vx // TILE
    pairs, per_pair = np.unique(tile_of.astype(np.int64) * F + face[vb, vk, vy, vx], return_counts=True)
    blended = np.bincount(pairs // F, weights=per_pair, minlength=nt).astype(np.int64)
    used = np.bincount(pairs // F, weights=(per_pair + 3) // 4 * 4, minlength=nt).astype(np.int64)

    def binding_grads(zero=None):
        keep = 1.0 if zero is None else th.from_numpy(~zero).to(gc.dtype)[:, None]
        g = _C.render_tris_backward(*args, (gc * keep).to(hip_device), (gd * keep).to(hip_device), out[0], *out[3:7])
        return dict(zip(TRI_GRADS, g))

    whole = binding_grads()
    runs = {}
    for fill, (body, out_bits) in FILLS.items():
        calls = GuardedCalls(hip_device, body, out_bits)
        lib = calls.lib
        lib.dmr_overflowed(-1, 1)
        tri_step(calls, small, H, W, 0)                       # leaves the estimate (few pairs per face) and a placement
        f, n = checked(calls, "tri_forward", big, H, W, 0, (0, 0), lambda: calls.tri_forward(big, H, W, 0))
        assert f.placed, ("the call before left a placement", n)
        assert f.R == out[0] and not lib.dmr_overflowed(-1, 1)
        b, _ = checked(calls, "tri_backward", big, H, W, capi.FLAG_ASYNC, (0, 0),
                       lambda: calls.tri_backward(big, H, W, capi.FLAG_ASYNC, f.R, gc, gd), R=f.R)   # (the guards are checked in there)
        assert lib.dmr_overflowed(-1, 1), "records beyond the capacity must be flagged"
        # The capacity, from the header's footprint of the work space: 32 BP + 8 BF + 8192 Nt + 16 per hit record, each rounded up
        # to 256 -- so what is derived here is the capacity rounded up to a multiple of 16 (the remainder is 0 by construction).
        # Region starts and whole blocks are multiples of 256: `end > capacity` is decided alike by the true and the derived value
        # unless the derived one is itself a multiple of 256, which is asserted not to be the case.
        work = dict(b.log)[capi.BUF_WORK]
        capacity = (work - up(32 * B * P) - up(8 * B * F) - 8192 * nt) // 16
        assert capacity % 256 != 0, capacity
        bufs = [calls.buffers[w] for w in range(4)]
        ex = lambda name: _C.export(name, f.args, False, f.R, bufs, H, W, th.int32).cpu().numpy().view(np.uint32).astype(np.int64)
        hits, ranges = ex("tile_hits"), ex("ranges").reshape(-1, 2)
        np.testing.assert_array_equal(hits, blended)
        lens = ranges[:, 1] - ranges[:, 0]
        bound = np.where(hits > 0, (hits + 3 * np.minimum(lens, hits) + 255) // 256 * 256, 0)   # record_bound, dmr_kernels.hpp
        start = np.cumsum(bound) - bound
        assert bool((used <= bound).all()) and 0 < capacity < int(bound.sum()), (capacity, int(bound.sum()))
        dropped = (used > 0) & (start + (used + 255) // 256 * 256 > capacity)   # k_tri_backward_hits' own test
        straddles = (used > 0) & (start < capacity) & (start + bound > capacity)
        assert dropped.any() and (~dropped & (used > 0)).any()
        got = dict(zip(TRI_GRADS, b.grads))
        # the default call repairs it: refuted, redone once (before the binding's call below refreshes the estimate)
        redo0 = lib.dmr_redo_count()
        b2, _ = checked(calls, "tri_backward", big, H, W, 0, (0, 0), lambda: calls.tri_backward(big, H, W, 0, f.R, gc, gd), R=f.R)
        assert lib.dmr_redo_count() == redo0 + 1 and [w for w, _ in b2.log].count(capi.BUF_WORK) == 2 and not lib.dmr_overflowed(-1, 1)
        e2 = close_grads(dict(zip(TRI_GRADS, b2.grads)), whole, (fill, "default after async"))
        e1 = close_grads(got, binding_grads(tile_pixels(dropped, B, H, W)), (fill, "async against the masked default call"))
        fate = "none" if not straddles.any() else "dropped" if bool(dropped[straddles].all()) else "kept"
        print(f"\ntri async backward ({fill}): placed forward {'redone' if len([1 for w, _ in f.log if w == capi.BUF_BINNING]) == 2 else 'fits'}; "
              f"capacity {capacity} of {int(bound.sum())} records ({int(used.sum())} used), {int(dropped.sum())} of {int((used > 0).sum())} busy tiles "
              f"dropped, straddling tile {fate}; gradients vs the masked default call {e1:.2e}; the default call after it {e2:.2e}")
        runs[fill] = (got, dict(zip(TRI_GRADS, b2.grads)))
    for a, b in zip(runs["zero"], runs["poison"]):
        close_grads(a, b, "tri async, zero vs poison")


# ---- f: idle calls -------------------------------------------------------------------------------------------------------------
def without(d, verts=False, faces=False):
    """d with no vertices / no faces (a tet mesh without faces has no tets; one without vertices has neither)"""
    d = dict(d)
    if verts:
        d.update(verts=d["verts"][:0], verts_color=d["verts_color"][:0], verts_depth=d["verts_depth"][:, :0])
        faces = faces or "tets" in d
    if faces:
        d.update(faces=d["faces"][:0], faces_opacity=d["faces_opacity"][:0], faces_intense=d["faces_intense"][:, :0])
        if "tets" in d:
            d.update(tets=d["tets"][:0], tet_faces=d["tet_faces"][:0], face_tets=d["face_tets"][:0])
    return d


@pytest.mark.parametrize("case", ["P0", "F0", "empty_band"])
def test_tri_idle_calls(hip_device, case):
    """Every flag set; nothing to render: P == 0 and F == 0 request nothing and return 0, an empty band requests its scratch and
    the fragment buffer; all outputs keep the pre-fill.  The backward zeroes every gradient (the camera gradients, requested all
    the same, included) and does not request the fragment inputs.  Launches, by the library's per-stage counters: none in the
    P == 0 / F == 0 forwards and in every idle backward; an empty band's forward runs its front end (it has geometry)."""
    import capi_ctypes as capi
    flags = tri_flag_sets(capi)["all"]
    d, H, W = tri_scene(), TRI["H"], TRI["W"]
    d = without(d, verts=True) if case == "P0" else without(d, faces=True) if case == "F0" else d
    rows = EMPTY_BAND if case == "empty_band" else (0, 0)
    for fill, (body, out_bits) in FILLS.items():
        calls = GuardedCalls(hip_device, body, out_bits)
        calls.inputs = {}
        r = _idle_tri(calls, d, H, W, flags, rows)
        assert r["R"] == 0
        nf, nb = r["launches"]
        assert sum(nb.values()) == 0, nb            # the idle backward: memsets, no kernel of any stage
        if case != "empty_band":                    # nothing is launched at all
            assert r["fwd"].log == [] and sum(nf.values()) == 0, nf
        else:                                       # the front end runs (there is geometry), no compositing kernel has a tile
            assert nf["k_tri_forward"] <= 1 and nf["k_project_verts"] == 1, nf
        for k, t in r["images"].items():
            assert th.equal(bits(t), bits(calls.prefill(t))), (case, fill, k)
        for k, t in r["grads"].items():
            assert float(t.abs().max()) == 0.0 if t.numel() else True, (case, fill, k)
        assert sorted(r["grads"]) == sorted(TRI_GRADS + ("inv_mv", "inv_proj"))
        print(f"\ntri idle {case} ({fill}): forward requests {[capi.BUF_NAMES[w] for w, _ in r['fwd'].log]}, backward requests "
              f"{[capi.BUF_NAMES[w] for w, _ in r['bwd'].log]}")


def _idle_tri(calls, d, H, W, flags, rows):
    """tri_step with no inputs registered: an idle backward must not ask for them (the callback would refuse, the call fail)"""
    capi = calls.capi
    B, P, F = d["mv_mats"].shape[0], d["verts"].shape[0], d["faces"].shape[0]
    gc, gd = upstream(B, H, W, True)
    f, nf = checked(calls, "tri_forward", d, H, W, flags, rows, lambda: calls.tri_forward(d, H, W, flags, rows))
    images = {"color": f.color, "depth": f.depth}
    if f.fragments is not None:
        images.update(unpack_fragments(f.fragments, B, H, W))
    b, nb = checked(calls, "tri_backward", d, H, W, flags, rows, lambda: calls.tri_backward(d, H, W, flags, f.R, gc, gd, rows), R=f.R)
    grads = dict(zip(TRI_GRADS, b.grads))
    grads.update(unpack_mats(b.camera, B, ("inv_mv", "inv_proj")))
    return {"R": f.R, "images": images, "grads": grads, "fwd": f, "bwd": b, "launches": (nf, nb)}


@pytest.mark.parametrize("case", ["P0", "F0", "empty_band"])
def test_tet_idle_calls(hip_device, case):
    """Every flag set.  An empty band: the scratch and the fragment buffer are requested, every output keeps the pre-fill.
    P == 0 / F == 0: the fragment buffer is not requested; the forward is not idle by the header -- nothing marches, and every
    pixel is written background / 1 / 0 (alpha 0).  The backward zeroes every gradient it owns and requests neither the fragment
    inputs nor the work space."""
    import capi_ctypes as capi
    flags = tet_flag_sets(capi)["all"]
    d, B, H, W = tet_scene(), TET["B"], TET["H"], TET["W"]
    d = without(d, verts=True) if case == "P0" else without(d, faces=True) if case == "F0" else d
    rows = EMPTY_BAND if case == "empty_band" else (0, 0)
    P, F = d["verts"].shape[0], d["faces"].shape[0]
    gc, gd = upstream(B, H, W, True)
    for fill, (body, out_bits) in FILLS.items():
        calls = GuardedCalls(hip_device, body, out_bits)
        calls.inputs = {}
        f, nf = checked(calls, "tet_forward", d, H, W, flags, rows, lambda: calls.tet_forward(d, H, W, flags, rows))
        assert f.R == 0
        assert (nf["k_tet_forward"] == 0) == (case == "empty_band"), nf   # an empty band marches nothing; P == 0 / F == 0 launch
        images = {"color": f.color, "depth": f.depth, "active": f.active}
        if case == "empty_band":
            images.update(unpack_fragments(f.fragments, B, H, W))
            for k, t in images.items():
                assert th.equal(bits(t), bits(calls.prefill(t))), (case, fill, k)
        else:
            assert f.fragments is None
            bg = th.tensor(BG, device=hip_device).view(1, 3, 1, 1).expand(B, 3, H, W)
            assert th.equal(f.color, bg) and float(f.active.abs().max()) == 0.0
            assert bool((f.depth[:, 0] == 1.0).all()) and bool((f.depth[:, 1] == 0.0).all())
        b, nb = checked(calls, "tet_backward", d, H, W, flags, rows, lambda: calls.tet_backward(d, H, W, flags, gc, gd, rows))
        assert sum(nb.values()) == 0, nb   # no kernel of any timed stage (the gradients are zeroed by an untimed fill)
        grads = dict(zip(TET_GRADS, b.grads))
        if b.full is not None:
            grads.update(unpack_tet_grads(b.full, P, B, F))
        grads.update(unpack_mats(b.camera, B, ("inv_mv", "inv_proj", "mv", "proj")))
        for k, t in grads.items():
            assert float(t.abs().max()) == 0.0 if t.numel() else True, (case, fill, k)
        print(f"\ntet idle {case} ({fill}): forward requests {[(capi.BUF_NAMES[w], n) for w, n in f.log]}, backward requests "
              f"{[capi.BUF_NAMES[w] for w, _ in b.log]}")
