"""Gradients of the tet fragment lists' barycentrics on the GPU (DMR_FLAG_TET_FRAGMENT_GRADS; `fragment_grads=(pix_to_face,
grad_bary)` of _C.render_tets_backward; TetRenderer(..., return_fragments=K, fragment_grads=True)) against the float64 model
of tests/tet_fragment_grads_ref.py.

Bounds (the project's own, tests/grad_cases.py and tests/util.py): dL_dverts rel_err <= TET_VERTS_TOL = 1e-3, the Module
matrices' gradients <= MATS_TOL = 1e-3, two evaluations of the same sums in another order <= sum_order_tol(name).  rel_err
divides by max(1, max|ref|): every comparison also asserts max|ref| >= 1, so that the bound is relative.  Pairs whose ray
grazes its face (grazing measure below 1e-2, den == 0 among them) carry no upstream, on both sides (the model's selection rule).
Every case prints what it measured (pytest -s).
"""
import numpy as np
import pytest
import torch as th

import tet_fragment_grads_ref as TFG
from fragments_ref import band_rows
from grad_cases import MATS_TOL, TET_VERTS_TOL, module_mats, scene
from harness import TET_ARGS, capture_replay, replay
from tet_camera_grad_ref import TetCameraGradRef
from util import c_args, rel_err, sum_order_tol, upstream_grads

pytestmark = pytest.mark.gpu

TET_NAMES = ("verts", "verts_color", "faces_opacity", "faces_intense", "verts", "verts", "mv", "proj")  # render_tets_backward's tuple
LEVELS = ({"full_grads": True}, {"camera_grads": True})


def _rel(got, ref, what):
    """rel_err with the bound made relative: the reference's largest entry must be at least 1."""
    ref = np.asarray(ref)
    big = float(np.abs(ref).max())
    assert big >= 1.0, (what, big)
    return rel_err(np.asarray(got), ref)


def _zeros(B, H, W, dev):
    return th.zeros(B, 3, H, W, device=dev), th.zeros(B, 1, H, W, device=dev)


def _np(g):
    return [x.cpu().numpy() for x in g]


def _check(g, rg, args, tag):
    """dL_dverts (and, level 2, the Module matrices' gradients) of a backward with zero image upstream against the model; every
    other gradient exactly 0."""
    ev = _rel(g[0].cpu().numpy(), rg["verts"], "verts")
    print(f"\n{tag}: dL_dverts {ev:.2e} (max |ref| {np.abs(rg['verts']).max():.3g})", end="")
    assert ev <= TET_VERTS_TOL, (tag, ev)
    for i in (1, 2, 3):  # dL_dverts_color, dL_dfaces_opacity, dL_dfaces_intense
        assert float(g[i].abs().max()) == 0.0, (tag, i)
    if len(g) == 8:
        assert float(g[6].abs().max()) == 0.0 and float(g[7].abs().max()) == 0.0, "(u, v) read the inverse matrices only"
        gm, gp = module_mats(args, g)
        em, ep = _rel(gm, rg["mv_mats"], "mv_mats"), _rel(gp, rg["proj_mats"], "proj_mats")
        print(f"  dL_dmv_mats {em:.2e} dL_dproj_mats {ep:.2e} (max |ref| {np.abs(rg['mv_mats']).max():.3g}, {np.abs(rg['proj_mats']).max():.3g})", end="")
        assert em <= MATS_TOL and ep <= MATS_TOL, (tag, em, ep)
    print()


@pytest.fixture(scope="module")
def synthetic():
    """Test 1's pairs and the model's gradients, computed once."""
    d, B, H, W, K, face, gb, pairs, g, dropped = TFG.synthetic()
    return d, B, H, W, K, face, gb, pairs, dropped, pairs.grads(g)


def test_synthetic_pairs(hip_device, synthetic):
    """Face ids drawn uniformly from [-1, F) on a 40 x 56 frame of two views (ragged in both directions): the pairs are the
    caller's, most rays miss their face (|u| up to 351).  Zero image upstream, at full_grads and at camera_grads.
    Measured on the MI355X: dL_dverts 5.0e-6 at both levels (max |ref| 5.9e4), dL_dmv_mats 3.1e-6, dL_dproj_mats 3.8e-6 (max
    |ref| 5.9e4, 3.7e5) -- what the same formula gives through float32 torch autograd (tests/test_tet_fragment_grads_cpu.py);
    ids outside [0, F) against a zeroed upstream: 3.4e-7 on dL_dverts, 0 on the inverse matrices' pieces."""
    from dmesh_renderer_amd import _C
    d, B, H, W, K, face, gb, pairs, dropped, rg = synthetic
    dev = hip_device
    assert int(dropped.sum()) <= 0.02 * len(pairs.u)
    args = c_args(d, dev, tet=True)
    zc, zd = _zeros(B, H, W, dev)
    faced, gbd = face.to(dev), gb.to(dev)
    out = _C.render_tets(*args, H, W, 0)  # (for the scratch buffers: the face records, the seed and the matrices live there)
    F = d["faces"].shape[0]
    for kw in LEVELS:
        g = _C.render_tets_backward(*args, zc, zd, *out[3:7], fragment_grads=(faced, gbd), **kw)
        assert len(g) == (8 if "camera_grads" in kw else 4)
        _check(g, rg, args, f"synthetic {kw}: {len(pairs.u)} pairs, {int(dropped.sum())} grazing")
    # the keyword alone raises the level to full_grads: its tuple
    g = _C.render_tets_backward(*args, zc, zd, *out[3:7], fragment_grads=(faced, gbd))
    assert len(g) == 4 and _rel(g[0].cpu().numpy(), rg["verts"], "verts") <= TET_VERTS_TOL
    # slots with ids -1, F and F + 7 written by hand = zeroing their upstream
    gen = th.Generator().manual_seed(5)
    hit = th.rand(face.shape, generator=gen) < 0.25
    bad = th.tensor([-1, F, F + 7], dtype=th.int32)[th.randint(0, 3, face.shape, generator=gen)]
    assert int((hit & (face >= 0)).sum()) > 1000
    f_bad = th.where(hit, bad, face).to(dev)
    g_zero = (gb * (~hit)[:, :, None].to(gb.dtype)).to(dev)
    a = _C.render_tets_backward(*args, zc, zd, *out[3:7], fragment_grads=(f_bad, gbd), camera_grads=True)
    b = _C.render_tets_backward(*args, zc, zd, *out[3:7], fragment_grads=(faced, g_zero), camera_grads=True)
    for i, name in ((0, "verts"), (4, "inv_mv"), (5, "inv_proj")):
        e = _rel(a[i].cpu().numpy(), b[i].cpu().numpy(), name)
        print(f"ids outside [0, F) vs zeroed upstream, {name}: {e:.2e}")
        assert e <= sum_order_tol("verts"), (name, e)


def test_edge_on_pair_with_an_upstream_contributes_nothing(hip_device, synthetic):
    """The kernel's denom == 0 skip with a NON-zero upstream (the model's selection rule zeroes the upstream of the set's own
    den == 0 pairs, so they never get that far).  One more face, (a, a, b), which nothing marches: E1 = p1 - p0 is exactly 0, so
    denom = (d x E2) . E1 is exactly 0 for every ray, in any precision.  A tenth of the slots get that face and keep an N(0, 1)
    upstream; the result must be the call with those slots' upstream zeroed -- without the skip 1 / denom is inf and the
    sums are NaN.  Measured on the MI355X: 1 333 such pairs, dL_dverts 6.3e-7, the inverse matrices' pieces 0."""
    from dmesh_renderer_amd import _C
    d0, B, H, W, K, face, gb, pairs, dropped, rg = synthetic
    dev = hip_device
    d = dict(d0)
    F = d0["faces"].shape[0]
    a, b = int(d0["faces"][0, 0]), int(d0["faces"][0, 1])
    d["faces"] = th.cat([d0["faces"], th.tensor([[a, a, b]], dtype=d0["faces"].dtype)])
    d["faces_opacity"] = th.cat([d0["faces_opacity"], d0["faces_opacity"][:1]])
    d["faces_intense"] = th.cat([d0["faces_intense"], d0["faces_intense"][:, :1]], 1)
    d["face_tets"] = th.cat([d0["face_tets"], th.full((1, 2), -1, dtype=d0["face_tets"].dtype)])
    args = c_args(d, dev, tet=True)
    zc, zd = _zeros(B, H, W, dev)
    out = _C.render_tets(*args, H, W, 0)
    gen = th.Generator().manual_seed(21)
    hit = th.rand(face.shape, generator=gen) < 0.1
    f_edge = th.where(hit, th.full_like(face, F), face).to(dev)
    g_live = th.where(hit[:, :, None], th.randn(gb.shape, generator=gen), gb)
    g_zero = th.where(hit[:, :, None], th.zeros_like(gb), gb)
    assert int(hit.sum()) > 1000 and bool((g_live[:, :, 0][hit] != 0).all())
    x = _C.render_tets_backward(*args, zc, zd, *out[3:7], fragment_grads=(f_edge, g_live.to(dev)), camera_grads=True)
    y = _C.render_tets_backward(*args, zc, zd, *out[3:7], fragment_grads=(f_edge, g_zero.to(dev)), camera_grads=True)
    for i, name in ((0, "verts"), (4, "inv_mv"), (5, "inv_proj")):
        assert bool(th.isfinite(x[i]).all()), name
        e = _rel(x[i].cpu().numpy(), y[i].cpu().numpy(), name)
        print(f"\n{int(hit.sum())} edge-on pairs with an upstream vs the same pairs without, {name}: {e:.2e}")
        assert e <= sum_order_tol("verts"), (name, e)


def test_full_table_faces_leave_directly(hip_device):
    """The kernel's full-table fallback: a pair whose face finds no slot adds its nine values to dL_dverts with float atomics.
    One 16 x 16 image (one tile), K = 4, caller-made pairs on the synthetic test's scene: the 1024 slots hold a permutation of
    its 864 faces (the rest unused), so no two lanes share a face for the merge to combine and the tile references nearly
    twice the faces its table has slots for.  Same model, same bounds as the synthetic test.  Measured on the MI355X: 848
    pairs (16 more graze), dL_dverts 5.7e-6 at both levels (max |ref| 5.8e4), dL_dmv_mats 3.1e-6, dL_dproj_mats 3.4e-6."""
    from dmesh_renderer_amd import _C, scenes
    TET_FRAG_TBL = 448  # dmr_tet.hip: TET_FRAG_TBL, the face slots of a workgroup's table (k_tet_fragment_grads' TetFragGradLds)
    dev = hip_device
    s = TFG.SYNTH
    B, H, W, K = 1, 16, 16, 4
    d = scenes.kuhn_tets(s["m"], B, H, W, seed=s["scene_seed"], opacity=s["opacity"])
    F = d["faces"].shape[0]
    assert F == 864
    gen = th.Generator().manual_seed(23)
    ids = th.cat([th.randperm(F, generator=gen), th.full((B * K * H * W - F,), -1, dtype=th.int64)])
    face = ids[th.randperm(len(ids), generator=gen)].reshape(B, K, H, W)
    pairs, where = TFG.pairs_of_lists(d, H, W, face)
    gb, g, dropped = TFG.masked_upstream((B, K, 2, H, W), pairs, where, gen)
    live = (g != 0).any(1).numpy()
    rows = np.unique(pairs.face.numpy()[live])  # (a row of this table is a face)
    assert len(rows) > 1.5 * TET_FRAG_TBL, len(rows)
    rg = pairs.grads(g)
    args = c_args(d, dev, tet=True)
    zc, zd = _zeros(B, H, W, dev)
    out = _C.render_tets(*args, H, W, 0)
    for kw in LEVELS:
        gk = _C.render_tets_backward(*args, zc, zd, *out[3:7], fragment_grads=(face.int().to(dev), gb.to(dev)), **kw)
        _check(gk, rg, args, f"full table {kw}: {int(live.sum())} pairs, {len(rows)} faces in the tile, {int(dropped.sum())} grazing")


_refs = {}
# W_extra / 16 that no other test of the suite gives the case (grad_cases.scene): view configurations of this file's own
OWN_WIDTHS = {"two_views_ragged": (1, 3), "opaque": (1, 2), "jitter": (1, 2)}


def _reference(oracle, case, W_extra=0):
    """The scene of a TET_CASES entry (widened: a view configuration of its own), the float64 model's kept pixels and every
    pixel's ndc sample (the pixel centre; a jittered scene's: the model's recovered sample on the kept pixels): computed once."""
    key = (case, W_extra)
    if key not in _refs:
        d, B, H, W, seed = scene(case, W_extra=W_extra)
        _, _, _, ost = oracle.tet_forward(oracle.scene_from_module_inputs(d, H, W, seed=seed))
        ref = TetCameraGradRef(d, H, W, ost, seed=seed)
        assert ref.kept_fraction >= 0.8, ref.kept_fraction
        ys, xs = th.meshgrid(th.arange(H), th.arange(W), indexing="ij")
        ndc = TFG.pixel_centres(xs.reshape(-1), ys.reshape(-1), H, W).repeat(B, 1)
        ndc[ref.pix] = ref.ndc
        _refs[key] = (d, B, H, W, seed, ref, ndc.reshape(B, H, W, 2))
    return _refs[key]


def _list_upstream(d, B, H, W, K, face, pixels, ndc, seed):
    """A random upstream on the pairs of the lists `face` on the pixels `pixels`, and the model's gradients for it."""
    pairs, where = TFG.pairs_of_lists(d, H, W, face, pixels, ndc)
    gb, g, dropped = TFG.masked_upstream((B, K, 2, H, W), pairs, where, th.Generator().manual_seed(seed))
    assert len(pairs.u) > 1000 and int(dropped.sum()) <= 0.01 * len(pairs.u), (len(pairs.u), int(dropped.sum()))
    return gb, pairs, g, dropped


@pytest.mark.parametrize("K", (8, 32))
@pytest.mark.parametrize("case", ("two_views_ragged", "opaque", "jitter"))
def test_rasterised_lists_match_float64_model(oracle, hip_device, case, K):
    """The lists the forward returns -- K = 8 truncates the deeper pixels, K = 32 holds every march (the longest is 28) -- on
    call 0 and call 1 of a view configuration of the case's and K's own (call 0: the re-marching backward runs ahead of the
    kernel at K = 8, the sequence one at K = 32), with a random upstream on the pixels the float64 model keeps.
    Measured on the MI355X (dL_dverts; dL_dmv_mats / dL_dproj_mats; pairs, of which grazing; both calls alike):
      two_views_ragged  K 8  8.1e-6; 1.6e-6 / 7.0e-7  (128 387, 1; 53 % of the pixels deeper than 8)   K 32  4.4e-6; 4.5e-7 / 7.8e-7  (210 453, 5)
      opaque            K 8  4.0e-6; 8.7e-7 / 1.4e-7  (22 365, 1; the longest march is 8)              K 32  3.0e-6; 6.4e-7 / 1.2e-7  (22 365, 1)
      jitter            K 8  1.1e-5; 6.1e-7 / 3.9e-7  (112 248, 2; 52 %)                               K 32  5.3e-6; 3.2e-6 / 4.3e-6  (183 897, 4)"""
    from dmesh_renderer_amd import _C
    dev = hip_device
    d, B, H, W, seed, ref, ndc = _reference(oracle, case, W_extra=16 * OWN_WIDTHS[case][K == 32])
    args = c_args(d, dev, tet=True)
    zc, zd = _zeros(B, H, W, dev)
    first = None
    for call in range(2):
        out = _C.render_tets(*args, H, W, seed, fragments=K)
        face = out[7].cpu()
        if first is None:
            first = face
            count = out[9].cpu()
            deeper = float((count > K).sum()) / max(1, int((count > 0).sum()))
            print(f"\n{case} K {K}: {100 * deeper:.0f} % of the pixels with fragments are deeper than K (longest march {int(count.max())})")
            # ("opaque" marches 8 faces at the most: its K = 8 lists are whole)
            assert (deeper > 0 or case == "opaque") if K == 8 else deeper == 0
            gb, pairs, g, dropped = _list_upstream(d, B, H, W, K, face, ref.mask()[:, 0], ndc, 7)
            rg, gbd = pairs.grads(g), gb.to(dev)
        assert th.equal(face, first)
        for kw in LEVELS:
            gk = _C.render_tets_backward(*args, zc, zd, *out[3:7], fragment_grads=(out[7], gbd), **kw)
            _check(gk, rg, args, f"{case} K {K} call {call} {kw}: {len(pairs.u)} pairs, {int(dropped.sum())} grazing")


def test_band(oracle, hip_device):
    """rows = (1, 4) on "small": the upstream on the band's kept pixels only, the lists the band call's."""
    from dmesh_renderer_amd import _C
    dev = hip_device
    K, rows = 8, (1, 4)
    d, B, H, W, seed, ref, ndc = _reference(oracle, "small")
    args = c_args(d, dev, tet=True)
    zc, zd = _zeros(B, H, W, dev)
    out = _C.render_tets(*args, H, W, seed, rows=rows, fragments=K)
    m = ref.mask()[:, 0] * th.from_numpy(band_rows(H, rows)).to(th.float32)[None, :, None]
    gb, pairs, g, dropped = _list_upstream(d, B, H, W, K, out[7].cpu(), m, ndc, 9)
    rg = pairs.grads(g)
    gk = _C.render_tets_backward(*args, zc, zd, *out[3:7], rows=rows, fragment_grads=(out[7], gb.to(dev)), camera_grads=True)
    _check(gk, rg, args, f"small rows {rows}: {len(pairs.u)} pairs")
    # a pixel outside the rendered rows contributes nothing: an upstream there changes nothing
    gen = th.Generator().manual_seed(10)
    outside = th.from_numpy(~band_rows(H, rows)).to(th.float32)[None, None, None, :, None]
    face_all = _C.render_tets(*args, H, W, seed, fragments=K)[7]
    g2 = _C.render_tets_backward(*args, zc, zd, *out[3:7], rows=rows,
                                 fragment_grads=(face_all, (gb + th.randn(B, K, 2, H, W, generator=gen) * outside).to(dev)), camera_grads=True)
    for i, name in ((0, "verts"), (4, "inv_mv"), (5, "inv_proj")):
        e = _rel(g2[i].cpu().numpy(), gk[i].cpu().numpy(), name)
        print(f"upstream outside the band, {name}: {e:.2e}")
        assert e <= sum_order_tol("verts"), (name, e)


def _warm_lists(dev, case, K, W_extra):
    """A warm view configuration of a case (two forwards, each with its backward, waited for: every later backward runs the
    sequence kernel, so two of them differ in summation order only), its K lists and an upstream on every stored pair that
    does not graze."""
    from dmesh_renderer_amd import _C
    d, B, H, W, seed = scene(case, W_extra=W_extra)
    args = c_args(d, dev, tet=True)
    gc, gd = (t.to(dev) for t in upstream_grads(B, H, W))
    for _ in range(2):
        out = _C.render_tets(*args, H, W, seed, fragments=K)
        _C.render_tets_backward(*args, gc, gd, *out[3:7])
        th.cuda.synchronize()  # (the backward leaves the next forward's estimate: from the second forward on, the sequence path)
    pairs, where = TFG.pairs_of_lists(d, H, W, out[7].cpu())
    gb, _, _ = TFG.masked_upstream((B, K, 2, H, W), pairs, where, th.Generator().manual_seed(3))
    return d, B, H, W, seed, args, gc, gd, out, gb.to(dev)


def test_additivity_and_nothing_else_moves(hip_device):
    """Image upstream and bary upstream together: dL_dverts and the inverse matrices' pieces = the call without the keyword +
    the keyword with zero image upstream; every other gradient is the call's without the keyword; a zero bary upstream is that
    call."""
    from dmesh_renderer_amd import _C
    dev = hip_device
    d, B, H, W, seed, args, gc, gd, out, gb = _warm_lists(dev, "two_views_ragged", 8, 16 * 4)
    zc, zd = _zeros(B, H, W, dev)
    pair = (out[7], gb)
    bw = lambda c, dd, **kw: _np(_C.render_tets_backward(*args, c, dd, *out[3:7], **kw))
    for kw in LEVELS:
        plain, only = bw(gc, gd, **kw), bw(zc, zd, fragment_grads=pair, **kw)
        both, zero = bw(gc, gd, fragment_grads=pair, **kw), bw(gc, gd, fragment_grads=(out[7], th.zeros_like(gb)), **kw)
        assert len(both) == len(plain) == (8 if "camera_grads" in kw else 4)
        assert np.abs(only[0]).max() >= 1.0, "the fragment term must be there"
        for i in [0] + ([4, 5] if len(both) == 8 else []):
            e = _rel(both[i], plain[i] + only[i], TET_NAMES[i])
            print(f"\n{kw} piece {i}: both vs plain + fragment-only {e:.2e}")
            assert e <= sum_order_tol("verts"), (i, e)
        for i, name in enumerate(TET_NAMES[:len(both)]):
            if i not in (0, 4, 5):
                eo = _rel(both[i], plain[i], name)
                assert eo <= sum_order_tol(name), (name, eo)
            ez = _rel(zero[i], plain[i], name)
            assert ez <= sum_order_tol(name), (name, ez)


def test_truncation(hip_device):
    """K = 2 lists with an upstream = K = 8 lists whose upstream is zero beyond slot 2 (pairs beyond K get nothing)."""
    from dmesh_renderer_amd import _C
    dev = hip_device
    d, B, H, W, seed, args, gc, gd, o8, g8 = _warm_lists(dev, "small", 8, 16 * 3)
    zc, zd = _zeros(B, H, W, dev)
    o2 = _C.render_tets(*args, H, W, seed, fragments=2)
    assert int((o8[9] > 2).sum()) > 0 and th.equal(o2[7], o8[7][:, :2])
    g2 = g8[:, :2].contiguous()
    g8 = g8.clone()
    g8[:, 2:] = 0
    a = _C.render_tets_backward(*args, zc, zd, *o2[3:7], fragment_grads=(o2[7], g2), camera_grads=True)
    b = _C.render_tets_backward(*args, zc, zd, *o8[3:7], fragment_grads=(o8[7], g8), camera_grads=True)
    for i, name in ((0, "verts"), (4, "inv_mv"), (5, "inv_proj")):
        e = _rel(a[i].cpu().numpy(), b[i].cpu().numpy(), name)
        print(f"\nK = 2 vs K = 8 with zeros beyond slot 2, {name}: {e:.2e}")
        assert e <= sum_order_tol("verts"), (name, e)


def test_module_through_autograd(oracle, hip_device):
    """A loss on fragments.interpolate(frag, faces, verts), the hit point, reaches verts, mv_mats and proj_mats as the FULL
    derivative of the hit point (the direct term through the vertex rows plus the (u, v) term); colour plus that loss is the
    sum of the two backwards; without fragment_grads bary does not require grad."""
    import dmesh_renderer_amd as dmr
    from dmesh_renderer_amd import fragments as FG
    dev = hip_device
    K = 8
    d, B, H, W, seed, ref, ndc = _reference(oracle, "two_views_ragged")
    gc, _ = upstream_grads(B, H, W)
    t = {k: v.to(dev) for k, v in d.items()}
    settings = dmr.TetRenderSettings(H, W, t["bg"], seed)
    names = ("verts", "mv_mats", "proj_mats")
    gcd = (gc * ref.mask()).to(dev)
    state = {}

    def step(color_loss, frag_loss, **opts):
        r = dmr.TetRenderer(settings, return_fragments=K, camera_grads=True, **opts)
        leaves = {k: t[k].clone().requires_grad_(True) for k in names}
        color, depth, active, frag = r(*(leaves.get(k, t[k]) for k in TET_ARGS))
        if "up" not in state:  # (the lists are the same on every call: the upstream is drawn once, on the kept pixels)
            pairs, where = TFG.pairs_of_lists(d, H, W, frag.pix_to_face.cpu(), ref.mask()[:, 0], ndc)
            b, k, y, x = where
            keep = ~pairs.grazes()
            up = th.zeros(B, K, 3, H, W)
            up[b[keep], k[keep], :, y[keep], x[keep]] = th.randn(int(keep.sum()), 3, generator=th.Generator().manual_seed(13))
            assert int((~keep).sum()) <= 0.01 * len(pairs.u)
            state.update(up=up.to(dev), pairs=pairs, rows=up[b, k, :, y, x].double())
        loss = 0
        if color_loss:
            loss = loss + (color * gcd).sum()
        if frag_loss:
            loss = loss + (FG.interpolate(frag, t["faces"], leaves["verts"]) * state["up"]).sum()
        loss.backward()
        return frag, {k: leaves[k].grad for k in names}

    frag, g_frag = step(False, True, fragment_grads=True)
    assert frag.bary.requires_grad and not frag.pix_to_face.requires_grad and not frag.count.requires_grad
    rg = state["pairs"].hit_grads(state["rows"])
    for kname, tol in (("verts", TET_VERTS_TOL), ("mv_mats", MATS_TOL), ("proj_mats", MATS_TOL)):
        e = _rel(g_frag[kname].cpu().numpy(), rg[kname], kname)
        print(f"\nModule, hit-point loss: dL_d{kname} {e:.2e} (max |ref| {np.abs(rg[kname]).max():.3g})")
        assert e <= tol, (kname, e)
    _, g_col = step(True, False, fragment_grads=True)   # (autograd delivers None for bary: the call without the term)
    _, g_both = step(True, True, fragment_grads=True)
    for kname in names:
        e = _rel(g_both[kname].cpu().numpy(), (g_col[kname] + g_frag[kname]).cpu().numpy(), kname)
        print(f"colour + hit-point loss vs the two backwards, dL_d{kname}: {e:.2e}")
        assert e <= sum_order_tol("verts"), (kname, e)  # (an identity, not a comparison with the model: the C-level test's bound)
    # without the option: bary is a constant, the loss reaches verts through the vertex rows only, the matrices not at all
    frag0, g_none = step(False, True)
    assert not frag0.bary.requires_grad and g_none["mv_mats"] is None and g_none["proj_mats"] is None
    assert _rel(g_none["verts"].cpu().numpy(), rg["verts"], "verts") > TET_VERTS_TOL, "the direct term alone is not the hit point's derivative"


def test_async_and_graph(hip_device):
    from dmesh_renderer_amd import _C
    dev = hip_device
    K = 8
    d, B, H, W, seed, args, gc, gd, out, gb = _warm_lists(dev, "small", K, 16 * 2)
    face = out[7].clone()
    want = [x.clone() for x in _C.render_tets_backward(*args, gc, gd, *out[3:7], fragment_grads=(face, gb), camera_grads=True)]
    assert float(want[0].abs().max()) >= 1.0
    _C.set_async(True)
    try:
        o = _C.render_tets(*args, H, W, seed)
        got = _C.render_tets_backward(*args, gc, gd, *o[3:7], fragment_grads=(face, gb), camera_grads=True)
        th.cuda.synchronize()
    finally:
        _C.set_async(False)
    assert not _C.overflowed()
    for name, a, b in zip(TET_NAMES, got, want):
        e = _rel(a.cpu().numpy(), b.cpu().numpy(), name)
        print(f"\nasync vs eager dL_d{name}: {e:.2e}")
        assert e <= sum_order_tol(name), (name, e)

    def step():
        o = _C.render_tets(*args, H, W, seed)
        return _C.render_tets_backward(*args, gc, gd, *o[3:7], fragment_grads=(face, gb), camera_grads=True)

    graph, captured, eager = capture_replay(step)
    for x in captured:
        x.zero_()
    replay(graph)
    for name, a, b in zip(TET_NAMES, captured, want):
        e = _rel(a.cpu().numpy(), b.cpu().numpy(), name)
        print(f"graph replay vs eager dL_d{name}: {e:.2e}")
        assert e <= sum_order_tol(name), (name, e)


def test_errors(hip_device):
    import dmesh_renderer_amd as dmr
    from dmesh_renderer_amd import _C
    from dmesh_renderer_amd.sharding import ShardedTetRenderer
    from dmesh_renderer_amd import scenes
    dev = hip_device
    m, B, H, W = 4, 1, 64, 80
    d = scenes.kuhn_tets(m, B, H, W, seed=0)
    args = c_args(d, dev, tet=True)
    zc, zd = _zeros(B, H, W, dev)
    out = _C.render_tets(*args, H, W, 0)
    face, gb = th.full((B, 2, H, W), -1, dtype=th.int32, device=dev), th.zeros(B, 2, 2, H, W, device=dev)

    def call(f, g):
        return _C.render_tets_backward(*args, zc, zd, *out[3:7], fragment_grads=(f, g))

    assert len(call(face, gb)) == 4
    for f, g, what in ((face.long(), gb, "int32"), (face, gb.double(), "float32"), (face[:, :, 1:], gb, "pix_to_face"),
                       (face, gb[:, :1], "grad_bary"), (face, gb[:, :, :1], "grad_bary"),
                       (face[:, :1].repeat(1, 33, 1, 1), gb[:, :1].repeat(1, 33, 1, 1, 1), "1..32"),
                       (face.cpu(), gb.cpu(), "must be on"), (face.transpose(2, 3), gb, "pix_to_face"),
                       # the right shapes, strided: only the contiguity check stands between these and a dense read
                       (th.full((B, 2, W, H), -1, dtype=th.int32, device=dev).transpose(2, 3), gb, "must be contiguous"),
                       (face, th.zeros(B, 2, 2, W, H, device=dev).transpose(3, 4), "must be contiguous"),
                       (face, th.zeros(B, 2, 2, H, 2 * W, device=dev)[..., ::2], "must be contiguous")):
        assert what != "must be contiguous" or (tuple(f.shape) == (B, 2, H, W) and tuple(g.shape) == (B, 2, 2, H, W)
                                                and not (f.is_contiguous() and g.is_contiguous()))
        with pytest.raises(RuntimeError, match="fragment_grads.*" + what):
            call(f, g)
    settings = dmr.TetRenderSettings(H, W, args[0], 0)
    with pytest.raises(ValueError, match="return_fragments"):
        dmr.TetRenderer(settings, fragment_grads=True)
    with pytest.raises(ValueError, match="return_fragments"):
        dmr.render_tet(*(d[k].to(dev) for k in TET_ARGS), settings, fragment_grads=True)
    with pytest.raises(ValueError, match="sharded"):
        ShardedTetRenderer(settings, fragment_grads=True)
