"""Gradients of the fragment lists' barycentrics on the GPU (DMR_FLAG_TRI_FRAGMENT_GRADS; `fragment_grads=(pix_to_face,
grad_bary)` of _C.render_tris_backward; TriRenderer(..., return_fragments=K, fragment_grads=True)) against the float64 model
of tests/fragment_grads_ref.py.

Bounds (the project's own, tests/grad_cases.py and tests/util.py): dL_dverts rel_err <= TRI_VERTS_TOL = 1e-4, the Module
matrices' gradients <= CAM_TOL = 1e-3, two evaluations of the same sums in another order <= sum_order_tol(name).  rel_err
divides by max(1, max|ref|): every comparison also asserts max|ref| >= 1, so that the bound is relative.  Every case prints
what it measured (pytest -s).
"""
import numpy as np
import pytest
import torch as th

import fragment_grads_ref as FGR
import fragments_ref as FR
from dmesh_renderer_amd import _through_inverse, scenes
from grad_cases import CAM_TOL, TRI_CASES, TRI_VERTS_TOL
from harness import TRI_ARGS, capture_replay, replay
from test_fragments_gpu import _deep_scene
from tri_grad_ref import TriGradRef
from util import c_args, rel_err, sum_order_tol, upstream_grads

pytestmark = pytest.mark.gpu

TRI_NAMES = ("verts", "verts_color", "faces_opacity", "verts_depth", "faces_intense")
LEVELS = ({}, {"exact_grads": True}, {"camera_grads": True})


def _rel(got, ref, what):
    """rel_err with the bound made relative: the reference's largest entry must be at least 1."""
    ref = np.asarray(ref)
    big = float(np.abs(ref).max())
    assert big >= 1.0, (what, big)
    return rel_err(np.asarray(got), ref)


def _module_mats(args, g):
    """dL/dmv_mats, dL/dproj_mats of the row-major Module matrices from a camera_grads backward's g[5:7] (gradients of the
    inverses of the transposed tensors args[5:7]): the chain through the inverse, transposed back."""
    return tuple(_through_inverse(args[7 + i], g[5 + i]).transpose(1, 2).cpu().numpy() for i in range(2))


def _zeros(B, H, W, dev):
    return th.zeros(B, 3, H, W, device=dev), th.zeros(B, 1, H, W, device=dev)


def _np(g):
    return [x.cpu().numpy() for x in g]


@pytest.fixture(scope="module")
def synthetic():
    """Test 1's pairs and the model's gradients, computed once.  The upstream is N(0, 1) on every pair but the ones within
    BORDER_EPS of a clamp border."""
    d, B, H, W, K, face, gb, pairs, g, dropped = FGR.synthetic()
    return d, B, H, W, K, face, gb, pairs, pairs.grads(g)


def test_synthetic_pairs_reach_every_clamp_region(hip_device, synthetic):
    """Face ids drawn uniformly from [-1, F): most rays miss their face, (u, v) reaches all seven regions of the clamp
    (|u| up to 67, |v| up to 98).  The backward takes the pairs from the caller, with zero image upstream, at all three levels.
    Measured on the MI355X with the unrestricted upstream (every pair but the 10 near a border; no restriction to
    max(|u|, |v|) <= 4 was needed): dL_dverts 1.3e-7 to 1.6e-7 at the three levels (max |ref| 345), dL_dmv_mats 2.8e-7,
    dL_dproj_mats 7.5e-8."""
    from dmesh_renderer_amd import _C
    d, B, H, W, K, face, gb, pairs, rg = synthetic
    dev = hip_device
    counts = np.bincount(pairs.region.numpy(), minlength=7)
    assert (counts >= 20).all(), counts
    args = c_args(d, dev)
    zc, zd = _zeros(B, H, W, dev)
    faced, gbd = face.to(dev), gb.to(dev)
    out = _C.render_tris(*args, H, W)  # (for the scratch buffers: the inverse matrices live in the image buffer)
    F = d["faces"].shape[0]
    for kw in LEVELS:
        g = _C.render_tris_backward(*args, zc, zd, out[0], *out[3:7], fragment_grads=(faced, gbd), **kw)
        ev = _rel(g[0].cpu().numpy(), rg["verts"], "verts")
        print(f"\nsynthetic {kw or 'reference level'}: {len(pairs.u)} pairs, regions {counts.tolist()}, dL_dverts {ev:.2e} "
              f"(max |ref| {np.abs(rg['verts']).max():.3g})")
        assert ev <= TRI_VERTS_TOL, (kw, ev)
        for i in range(1, 5):  # zero image upstream: nothing else receives anything
            assert float(g[i].abs().max()) == 0.0, (kw, i)
        if "camera_grads" in kw:
            gm, gp = _module_mats(args, g)
            em, ep = _rel(gm, rg["mv_mats"], "mv_mats"), _rel(gp, rg["proj_mats"], "proj_mats")
            print(f"synthetic: dL_dmv_mats {em:.2e} dL_dproj_mats {ep:.2e} (max |ref| {np.abs(rg['mv_mats']).max():.3g}, "
                  f"{np.abs(rg['proj_mats']).max():.3g})")
            assert em <= CAM_TOL and ep <= CAM_TOL, (em, ep)
    # slots with ids -1, F and F + 7 written by hand = zeroing their upstream
    gen = th.Generator().manual_seed(5)
    hit = th.rand(face.shape, generator=gen) < 0.25
    bad = th.tensor([-1, F, F + 7], dtype=th.int32)[th.randint(0, 3, face.shape, generator=gen)]
    assert int((hit & (face >= 0)).sum()) > 1000
    f_bad = th.where(hit, bad, face).to(dev)
    g_zero = (gb * (~hit)[:, :, None].to(gb.dtype)).to(dev)
    a = _C.render_tris_backward(*args, zc, zd, out[0], *out[3:7], fragment_grads=(f_bad, gbd), camera_grads=True)
    b = _C.render_tris_backward(*args, zc, zd, out[0], *out[3:7], fragment_grads=(faced, g_zero), camera_grads=True)
    for i, name in ((0, "verts"), (5, "inv_mv"), (6, "inv_proj")):
        e = _rel(a[i].cpu().numpy(), b[i].cpu().numpy(), name)
        print(f"ids outside [0, F) vs zeroed upstream, {name}: {e:.2e}")
        assert e <= sum_order_tol("verts"), (name, e)


def test_full_table_rows_leave_directly(hip_device):
    """The kernel's full-table fallback: a pair whose (view, vertex) row finds no slot adds its three values to the packed
    vertex rows with float atomics.  One 16 x 16 image (one tile), K = 3, caller-made pairs as in the synthetic test: its 768
    slots hold a permutation of the 768 faces of a six-sheet scene taken apart into a soup (P = 3 F: no two faces share a
    vertex), so the tile references three distinct rows per pair with an upstream, four times the table's slots.  Same
    model, same bounds as the synthetic test.  Measured on the MI355X: 768 pairs, 2304 rows, dL_dverts 4.8e-7 at the three
    levels (max |ref| 39.9), dL_dmv_mats 3.5e-7, dL_dproj_mats 2.2e-7."""
    from dmesh_renderer_amd import _C
    VTAB = 560  # dmr_tri.hip: VTAB, the vertex-row slots of a workgroup's table (k_tri_fragment_grads' FragGradLds)
    dev = hip_device
    B, H, W, K = 1, 16, 16, 3
    d = scenes.layered_sheets(6, 9, B, H, W, seed=7, opacity=(0.1, 0.5))
    vid = d["faces"].long().reshape(-1)
    F = d["faces"].shape[0]
    assert F == B * K * H * W
    d.update(verts=d["verts"][vid], verts_color=d["verts_color"][vid], verts_depth=d["verts_depth"][:, vid],
             faces=th.arange(3 * F, dtype=th.int32).reshape(F, 3))
    gen = th.Generator().manual_seed(23)
    face = th.randperm(F, generator=gen).reshape(B, K, H, W)
    gb = th.randn(B, K, 2, H, W, generator=gen)
    pairs, (b, k, y, x) = FGR.pairs_of_lists(d, H, W, face)
    keep = ~pairs.near_border()
    mask = th.zeros(B, K, H, W)
    mask[b, k, y, x] = keep.to(mask.dtype)
    gb = (gb * mask[:, :, None]).contiguous()
    live = (gb[b, k, :, y, x] != 0).any(1).numpy()
    rows = np.unique(d["faces"].numpy()[pairs.face.numpy()[live]])  # (one view, one tile: a row is a vertex)
    assert len(rows) > 2 * VTAB, len(rows)
    rg = pairs.grads(gb[b, k, :, y, x])
    args = c_args(d, dev)
    zc, zd = _zeros(B, H, W, dev)
    out = _C.render_tris(*args, H, W)
    for kw in LEVELS:
        g = _C.render_tris_backward(*args, zc, zd, out[0], *out[3:7], fragment_grads=(face.int().to(dev), gb.to(dev)), **kw)
        ev = _rel(g[0].cpu().numpy(), rg["verts"], "verts")
        print(f"\nfull table {kw or 'reference level'}: {int(live.sum())} pairs, {len(rows)} rows in the tile, dL_dverts {ev:.2e} "
              f"(max |ref| {np.abs(rg['verts']).max():.3g})")
        assert ev <= TRI_VERTS_TOL, (kw, ev)
        if "camera_grads" in kw:
            gm, gp = _module_mats(args, g)
            em, ep = _rel(gm, rg["mv_mats"], "mv_mats"), _rel(gp, rg["proj_mats"], "proj_mats")
            print(f"full table: dL_dmv_mats {em:.2e} dL_dproj_mats {ep:.2e} (max |ref| {np.abs(rg['mv_mats']).max():.3g}, "
                  f"{np.abs(rg['proj_mats']).max():.3g})")
            assert em <= CAM_TOL and ep <= CAM_TOL, (em, ep)


def _rasterised(oracle, dev, case):
    """A case of TRI_CASES: its K = 8 lists from render_tris(fragments=K) (confirmed to be the model's), a random upstream on
    the kept pixels of the band, the model's gradients for it."""
    from dmesh_renderer_amd import _C
    K = 8
    L, n, B, H, W, rows = TRI_CASES[case]
    d = scenes.layered_sheets(L, n, B, H, W, seed=7, opacity=(0.1, 0.5))  # (grad_cases.setup's scene, model and demand)
    ref = TriGradRef(d, H, W, oracle.tri_forward(oracle.scene_from_module_inputs(d, H, W))[2])
    assert ref.kept_fraction >= 0.8, ref.kept_fraction
    args = c_args(d, dev)
    out = _C.render_tris(*args, H, W, rows=rows, fragments=K)
    face, bary, count = (t.cpu() for t in out[7:10])
    FR.check_model(ref, d, face.numpy(), bary.numpy(), count.numpy(), rows)
    m = ref.mask()[:, 0] * th.from_numpy(FR.band_rows(H, rows)).to(th.float32)[None, :, None]  # [B,H,W]
    gen = th.Generator().manual_seed(7)
    gb = th.randn(B, K, 2, H, W, generator=gen) * m[:, None, None]
    pairs, (b, k, y, x) = FGR.pairs_of_lists(d, H, W, face, m)
    assert len(pairs.u) > 1000
    g = gb[b, k, :, y, x]
    # (a kept pixel's pairs are away from the clamp borders: TriGradRef drops pixels within CLAMP_EPS of one)
    return d, B, H, W, rows, K, args, gb, pairs.grads(g)


@pytest.mark.parametrize("case", list(TRI_CASES))
def test_rasterised_lists_match_float64_model(oracle, hip_device, case):
    """The lists the forward returns, on call 0 and call 1 of the view configuration."""
    from dmesh_renderer_amd import _C
    dev = hip_device
    d, B, H, W, rows, K, args, gb, rg = _rasterised(oracle, dev, case)
    zc, zd = _zeros(B, H, W, dev)
    gbd = gb.to(dev)
    for call in range(2):
        out = _C.render_tris(*args, H, W, rows=rows, fragments=K)
        g = _C.render_tris_backward(*args, zc, zd, out[0], *out[3:7], rows=rows, fragment_grads=(out[7], gbd), camera_grads=True)
        ge = _C.render_tris_backward(*args, zc, zd, out[0], *out[3:7], rows=rows, fragment_grads=(out[7], gbd), exact_grads=True)
        ev, ee = _rel(g[0].cpu().numpy(), rg["verts"], "verts"), _rel(ge[0].cpu().numpy(), rg["verts"], "verts")
        gm, gp = _module_mats(args, g)
        em, ep = _rel(gm, rg["mv_mats"], "mv_mats"), _rel(gp, rg["proj_mats"], "proj_mats")
        print(f"\n{case} call {call}: dL_dverts {ev:.2e} (exact level {ee:.2e}) dL_dmv_mats {em:.2e} dL_dproj_mats {ep:.2e}  "
              f"(max |ref| {np.abs(rg['verts']).max():.3g}, {np.abs(rg['mv_mats']).max():.3g}, {np.abs(rg['proj_mats']).max():.3g})")
        assert ev <= TRI_VERTS_TOL and ee <= TRI_VERTS_TOL, (ev, ee)
        assert em <= CAM_TOL and ep <= CAM_TOL, (em, ep)


def test_additivity_and_nothing_else_moves(hip_device):
    """Image upstream and bary upstream together: dL_dverts (and the camera piece) = the call without the flag + the flag with
    zero image upstream; the other four gradients are the call's without the flag; a zero bary upstream is that call."""
    from dmesh_renderer_amd import _C
    dev = hip_device
    K = 8
    L, n, B, H, W, rows = TRI_CASES["two_views_ragged"]
    d = scenes.layered_sheets(L, n, B, H, W, seed=7, opacity=(0.1, 0.5))
    args = c_args(d, dev)
    gc, gd = (t.to(dev) for t in upstream_grads(B, H, W))
    zc, zd = _zeros(B, H, W, dev)
    for _ in range(2):  # warm: every backward below runs on the same kind of forward state
        out = _C.render_tris(*args, H, W, fragments=K)
    gb = th.randn(B, K, 2, H, W, generator=th.Generator().manual_seed(3)).to(dev) * (out[7] >= 0)[:, :, None]
    pair = (out[7], gb)
    for kw in LEVELS:
        plain = _np(_C.render_tris_backward(*args, gc, gd, out[0], *out[3:7], **kw))
        only = _np(_C.render_tris_backward(*args, zc, zd, out[0], *out[3:7], fragment_grads=pair, **kw))
        both = _np(_C.render_tris_backward(*args, gc, gd, out[0], *out[3:7], fragment_grads=pair, **kw))
        zero = _np(_C.render_tris_backward(*args, gc, gd, out[0], *out[3:7], fragment_grads=(out[7], th.zeros_like(gb)), **kw))
        assert len(both) == len(plain) == (7 if "camera_grads" in kw else 5)
        assert np.abs(only[0]).max() >= 1.0, "the fragment term must be there"
        e = _rel(both[0], plain[0] + only[0], "verts")
        print(f"\n{kw or 'reference level'}: dL_dverts both vs plain + fragment-only {e:.2e}")
        assert e <= sum_order_tol("verts"), e
        for i in range(5, len(both)):
            ec = _rel(both[i], plain[i] + only[i], "camera")
            print(f"camera piece {i}: {ec:.2e}")
            assert ec <= sum_order_tol("verts"), (i, ec)
        for i, name in enumerate(TRI_NAMES):
            if i:
                eo = _rel(both[i], plain[i], name)
                assert eo <= sum_order_tol(name), (name, eo)
            ez = _rel(zero[i], plain[i], name)
            assert ez <= sum_order_tol(name), (name, ez)
        for i in range(5, len(both)):
            assert _rel(zero[i], plain[i], "camera") <= sum_order_tol("verts"), i


def test_truncation(hip_device):
    """K = 2 lists with an upstream = K = 8 lists whose upstream is zero beyond slot 2 (pairs beyond K get nothing)."""
    from dmesh_renderer_amd import _C
    dev = hip_device
    d, B, H, W = _deep_scene()
    args = c_args(d, dev)
    zc, zd = _zeros(B, H, W, dev)
    o8 = _C.render_tris(*args, H, W, fragments=8)
    o2 = _C.render_tris(*args, H, W, fragments=2)
    assert int((o8[9] > 2).sum()) > 0 and th.equal(o2[7], o8[7][:, :2])
    g2 = th.randn(B, 2, 2, H, W, generator=th.Generator().manual_seed(11)).to(dev)
    g8 = th.zeros(B, 8, 2, H, W, device=dev)
    g8[:, :2] = g2
    a = _C.render_tris_backward(*args, zc, zd, o2[0], *o2[3:7], fragment_grads=(o2[7], g2), camera_grads=True)
    b = _C.render_tris_backward(*args, zc, zd, o8[0], *o8[3:7], fragment_grads=(o8[7], g8), camera_grads=True)
    for i, name in ((0, "verts"), (5, "inv_mv"), (6, "inv_proj")):
        e = _rel(a[i].cpu().numpy(), b[i].cpu().numpy(), name)
        print(f"\nK = 2 vs K = 8 with zeros beyond slot 2, {name}: {e:.2e}")
        assert e <= sum_order_tol("verts"), (name, e)


def test_module_through_autograd(oracle, hip_device):
    """A loss on fragments.interpolate(frag, faces, attr) alone reaches verts, mv_mats and proj_mats; colour plus that term is
    the sum of the two backwards; without fragment_grads the same loss leaves verts.grad None."""
    import dmesh_renderer_amd as dmr
    from dmesh_renderer_amd import fragments as FG
    dev = hip_device
    case = "two_views_ragged"
    K = 8
    L, n, B, H, W, rows = TRI_CASES[case]
    d = scenes.layered_sheets(L, n, B, H, W, seed=7, opacity=(0.1, 0.5))
    ref = TriGradRef(d, H, W, oracle.tri_forward(oracle.scene_from_module_inputs(d, H, W))[2])
    assert ref.kept_fraction >= 0.8, ref.kept_fraction
    gc, _ = upstream_grads(B, H, W)
    t = {k: v.to(dev) for k, v in d.items()}
    settings = dmr.TriRenderSettings(H, W, t["bg"])
    names = ("verts", "mv_mats", "proj_mats")
    gen = th.Generator().manual_seed(13)
    attr = th.randn(d["verts"].shape[0], 4, generator=gen)
    up = th.randn(B, K, 4, H, W, generator=gen) * ref.mask()[:, None]  # (kept pixels only)
    attr_d, up_d, gcd = attr.to(dev), up.to(dev), (gc * ref.mask()).to(dev)

    def step(color_loss, frag_loss, **opts):
        r = dmr.TriRenderer(settings, return_fragments=K, exact_grads=True, camera_grads=True, **opts)
        leaves = {k: t[k].clone().requires_grad_(True) for k in names}
        a = attr_d.clone().requires_grad_(True)
        color, depth, frag = r(*(leaves.get(k, t[k]) for k in TRI_ARGS))
        loss = 0
        if color_loss:
            loss = loss + (color * gcd).sum()
        if frag_loss:
            loss = loss + (FG.interpolate(frag, t["faces"], a) * up_d).sum()
        loss.backward()
        return frag, {k: leaves[k].grad for k in names}

    frag, g_frag = step(False, True, fragment_grads=True)
    assert frag.bary.requires_grad and not frag.pix_to_face.requires_grad and not frag.count.requires_grad
    # the model: d loss / d(u_c, v_c) of a pair = up . (a_1 - a_0, a_2 - a_0)
    face = frag.pix_to_face.cpu()
    FR.check_model(ref, d, face.numpy(), frag.bary.detach().cpu().numpy(), frag.count.cpu().numpy())
    pairs, (b, k, y, x) = FGR.pairs_of_lists(d, H, W, face, ref.mask()[:, 0])
    vid = d["faces"].long()[pairs.face]
    a64, u64 = attr.double(), up.double()[b, k, :, y, x]
    g = th.stack([(u64 * (a64[vid[:, 1]] - a64[vid[:, 0]])).sum(1), (u64 * (a64[vid[:, 2]] - a64[vid[:, 0]])).sum(1)], 1)
    rg = pairs.grads(g)
    for kname, tol in (("verts", TRI_VERTS_TOL), ("mv_mats", CAM_TOL), ("proj_mats", CAM_TOL)):
        e = _rel(g_frag[kname].cpu().numpy(), rg[kname], kname)
        print(f"\nModule, interpolate loss: dL_d{kname} {e:.2e} (max |ref| {np.abs(rg[kname]).max():.3g})")
        assert e <= tol, (kname, e)
    _, g_col = step(True, False, fragment_grads=True)   # (autograd delivers None for bary: today's call)
    _, g_both = step(True, True, fragment_grads=True)
    for kname in names:
        e = _rel(g_both[kname].cpu().numpy(), (g_col[kname] + g_frag[kname]).cpu().numpy(), kname)
        print(f"colour + interpolate vs the two backwards, dL_d{kname}: {e:.2e}")
        assert e <= (sum_order_tol("verts") if kname == "verts" else CAM_TOL), (kname, e)
    frag0, g_none = step(False, True)
    assert not frag0.bary.requires_grad and all(g_none[k] is None for k in names)


def test_async_and_graph(hip_device):
    from dmesh_renderer_amd import _C
    dev = hip_device
    K = 8
    d, B, H, W = _deep_scene(W=176)  # (a view configuration of this test's own)
    args = c_args(d, dev)
    gc, gd = (t.to(dev) for t in upstream_grads(B, H, W))
    out = _C.render_tris(*args, H, W, fragments=K)
    face = out[7].clone()
    gb = th.randn(B, K, 2, H, W, generator=th.Generator().manual_seed(17)).to(dev)
    want = [x.clone() for x in _C.render_tris_backward(*args, gc, gd, out[0], *out[3:7], fragment_grads=(face, gb), camera_grads=True)]
    assert float(want[0].abs().max()) >= 1.0
    names = TRI_NAMES + ("verts", "verts")
    _C.set_async(True)
    try:
        o = _C.render_tris(*args, H, W)
        got = _C.render_tris_backward(*args, gc, gd, o[0], *o[3:7], fragment_grads=(face, gb), camera_grads=True)
        th.cuda.synchronize()
    finally:
        _C.set_async(False)
    assert not _C.overflowed()
    for name, a, b in zip(names, got, want):
        e = _rel(a.cpu().numpy(), b.cpu().numpy(), name)
        print(f"\nasync vs eager dL_d{name}: {e:.2e}")
        assert e <= sum_order_tol(name), (name, e)

    def step():
        o = _C.render_tris(*args, H, W)
        return _C.render_tris_backward(*args, gc, gd, o[0], *o[3:7], fragment_grads=(face, gb), camera_grads=True)

    graph, captured, eager = capture_replay(step)
    for x in captured:
        x.zero_()
    replay(graph)
    for name, a, b in zip(names, captured, want):
        e = _rel(a.cpu().numpy(), b.cpu().numpy(), name)
        print(f"graph replay vs eager dL_d{name}: {e:.2e}")
        assert e <= sum_order_tol(name), (name, e)


def test_errors(hip_device):
    import dmesh_renderer_amd as dmr
    from dmesh_renderer_amd import _C
    from dmesh_renderer_amd.sharding import ShardedTriRenderer
    dev = hip_device
    L, n, B, H, W, _ = TRI_CASES["one_view"]
    d = scenes.layered_sheets(L, n, B, H, W, seed=7)
    args = c_args(d, dev)
    zc, zd = _zeros(B, H, W, dev)
    out = _C.render_tris(*args, H, W)
    face, gb = th.full((B, 2, H, W), -1, dtype=th.int32, device=dev), th.zeros(B, 2, 2, H, W, device=dev)

    def call(f, g):
        return _C.render_tris_backward(*args, zc, zd, out[0], *out[3:7], fragment_grads=(f, g))

    assert len(call(face, gb)) == 5
    for f, g, what in ((face.long(), gb, "int32"), (face, gb.double(), "float32"), (face[:, :, 1:], gb, "pix_to_face"),
                       (face, gb[:, :1], "grad_bary"), (face, gb[:, :, :1], "grad_bary"),
                       (face[:, :1].repeat(1, 33, 1, 1), gb[:, :1].repeat(1, 33, 1, 1, 1), "1..32"),
                       (face.cpu(), gb.cpu(), "must be on"), (face.transpose(2, 3), gb, "pix_to_face")):
        with pytest.raises(RuntimeError, match="fragment_grads.*" + what):
            call(f, g)
    settings = dmr.TriRenderSettings(H, W, args[0])
    with pytest.raises(ValueError, match="return_fragments"):
        dmr.TriRenderer(settings, fragment_grads=True)
    with pytest.raises(ValueError, match="return_fragments"):
        dmr.render_tri(*(d[k].to(dev) for k in TRI_ARGS), settings, fragment_grads=True)
    with pytest.raises(ValueError, match="sharded"):
        ShardedTriRenderer(settings, fragment_grads=True)
