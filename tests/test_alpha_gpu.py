"""The alpha (coverage) output on the GPU (DMR_FLAG_ALPHA; `alpha=True` of the binding; return_alpha=True of the Modules)
against the CPU oracle, by the two identities of tests/alpha_ref.py:

  alpha == 1 - T (T the oracle's final transmittance), 0 where the tet march fails and outside a row band;
  dL_dfaces_opacity for upstream (g_c, g_d, g_a) == oracle(scene; g_c, g_d) + oracle(colourless twin; dL_dcolor[:, 0] = -g_a).

Bounds (the project's own): alpha 1e-5 absolute; gradients rel_err <= 1e-4; colour and the depth channel bit-identical to the
call without the flag; every gradient but faces_opacity within 1e-5 of the call without alpha.  Every case prints what it
measured (pytest -s); the figures taken on the MI355X are quoted in the README.
"""
import numpy as np
import pytest
import torch as th

import alpha_ref
from dmesh_renderer_amd import scenes
from grad_cases import TRI_CASES, seq_state
from harness import capture_replay, module_step, replay, run_ranks
from util import c_args, rel_err, upstream_grads

pytestmark = pytest.mark.gpu

FWD_TOL = 1e-5
GRAD_TOL = 1e-4
SAME_TOL = 1e-5

TET_CASES = {
    # name: (m, B, H, W, rows)
    "kuhn": (3, 2, 64, 96, (0, 0)),
    "kuhn_band": (3, 2, 64, 96, (1, 3)),
}
TRI_NAMES = ("verts", "verts_color", "faces_opacity", "verts_depth", "faces_intense")


def _upstream(B, H, W, rows, dev):
    """(g_c, g_d, g_a) on the CPU, zero outside the band, and (g_c, [g_d | g_a], g_d) on the device."""
    gc, gd = upstream_grads(B, H, W)
    ga = th.randn(B, 1, H, W, generator=th.Generator().manual_seed(5))
    m = th.from_numpy(alpha_ref.band_mask(H, rows))[None, None, :, None]
    gc, gd, ga = gc * m, gd * m, ga * m
    return gc, gd, ga, gc.to(dev), th.cat([gd, ga], dim=1).to(dev), gd.to(dev)


def _np(ts):
    return [x.cpu().numpy() for x in ts]


def _check_tri(oracle, dev, d, B, H, W, rows, tag, options=True):
    from dmesh_renderer_amd import _C
    sc = oracle.scene_from_module_inputs(d, H, W, rows=rows)
    _, _, ost = oracle.tri_forward(sc)
    gc, gd, ga, gcd, gdad, gdd = _upstream(B, H, W, rows, dev)
    want_alpha = alpha_ref.expected_alpha(sc, ost, False, rows)
    og = oracle.tri_backward(sc, ost, gc.numpy(), gd.numpy())
    want_fo = og["faces_opacity"] + alpha_ref.alpha_opacity_grad(sc, ga.numpy(), False, rows)
    assert np.abs(want_fo - og["faces_opacity"]).max() > 1e-2, "the alpha term must matter"
    args = c_args(d, dev)
    for call in range(2):  # the first backward of a view configuration (scanned record regions), then a later one
        outa = _C.render_tris(*args, H, W, rows=rows, alpha=True)
        gra = _np(_C.render_tris_backward(*args, gcd, gdad, outa[0], *outa[3:7], rows=rows, alpha=True))
        out0 = _C.render_tris(*args, H, W, rows=rows)
        gr0 = _np(_C.render_tris_backward(*args, gcd, gdd, out0[0], *out0[3:7], rows=rows))
        assert tuple(outa[2].shape) == (B, 2, H, W) and tuple(out0[2].shape) == (B, 1, H, W) and outa[0] == out0[0]
        assert th.equal(outa[1], out0[1]) and th.equal(outa[2][:, :1], out0[2]), "colour / depth must not change with the flag"
        ea = float(np.abs(outa[2][:, 1:].cpu().numpy() - want_alpha).max())
        ef = rel_err(gra[2], want_fo)
        print(f"\n{tag} call {call}: alpha {ea:.2e}  dL_dfaces_opacity {ef:.2e}  (without the alpha term {rel_err(gr0[2], want_fo):.2e})")
        assert ea <= FWD_TOL, ea
        assert ef <= GRAD_TOL, ef
        for i, k in enumerate(TRI_NAMES):
            if k != "faces_opacity":
                assert rel_err(gra[i], gr0[i]) <= SAME_TOL, k
                if k != "verts":  # (the reference's own verts gradient is compared in tests/test_tri_parity_gpu.py)
                    assert rel_err(gra[i], og[k]) <= GRAD_TOL, k
        if not options:
            continue
        for kw in ({"exact_grads": True}, {"camera_grads": True}):
            gka = _np(_C.render_tris_backward(*args, gcd, gdad, outa[0], *outa[3:7], rows=rows, alpha=True, **kw))
            gk0 = _np(_C.render_tris_backward(*args, gcd, gdd, out0[0], *out0[3:7], rows=rows, **kw))
            assert len(gka) == len(gk0)
            for i in range(len(gk0)):
                if i != 2:
                    assert rel_err(gka[i], gk0[i]) <= SAME_TOL, (kw, i)
            e = rel_err(gka[2], want_fo)
            print(f"{tag} call {call} {list(kw)[0]}: dL_dfaces_opacity {e:.2e}")
            assert e <= GRAD_TOL, (kw, e)
    return want_alpha


@pytest.mark.parametrize("case", list(TRI_CASES))
def test_tri_alpha_matches_oracle(oracle, hip_device, case):
    L, n, B, H, W, rows = TRI_CASES[case]
    d = scenes.layered_sheets(L, n, B, H, W, seed=7, opacity=(0.1, 0.5))
    a = _check_tri(oracle, hip_device, d, B, H, W, rows, case)
    assert a.max() > 0.3 and a.min() == 0.0
    if rows != (0, 0):
        assert (a[:, :, :16 * rows[0]] == 0).all() and (a[:, :, 16 * rows[1]:] == 0).all()


def test_tri_alpha_opaque_faces_and_early_stop(oracle, hip_device):
    """Faces of opacity 1 (the prev_T_final case) and a stack deep enough for the early stop T < T_EPS."""
    L, n, B, H, W = 14, 6, 1, 96, 144
    d = scenes.layered_sheets(L, n, B, H, W, seed=3, opacity=(0.45, 0.9))
    d["faces_opacity"][::11] = 1.0
    sc = oracle.scene_from_module_inputs(d, H, W)
    _, _, ost = oracle.tri_forward(sc)
    T = ost.get("final_T")
    assert (T == 0).any(), "a pixel must end on a face of opacity 1"
    assert ((T > 0) & (T < 1e-4)).any(), "a pixel must stop early (T < T_EPS)"
    assert (T == 1).any()
    _check_tri(oracle, hip_device, d, B, H, W, (0, 0), "opaque+deep")


def test_tri_alpha_scanned_path(oracle, hip_device):
    """A frame of more than 8 192 tiles (tests/test_tri_exact_grads_gpu.py::test_camera_grads_scanned_path's): the record
    regions come from k_scan_hits on every call, the forward runs on lists sorted by k_sort_tiles."""
    L, n, B, H, W = 3, 40, 1, 1040, 2048
    assert ((H + 15) // 16) * ((W + 15) // 16) * B > 8192
    d = scenes.layered_sheets(L, n, B, H, W, seed=5, opacity=(0.1, 0.5))
    d["verts"] = d["verts"] * th.tensor([4.0, 4.0, 1.0])
    _check_tri(oracle, hip_device, d, B, H, W, (0, 0), "scanned", options=False)


@pytest.mark.parametrize("case", list(TET_CASES))
def test_tet_alpha_matches_oracle(oracle, hip_device, case):
    """Call 0 is the first of its view configuration (no march sequence: the re-marching k_tet_backward), call 1 runs
    k_tet_backward_seq.  Inactive pixels: alpha exactly 0, and an upstream gradient there reaches nothing."""
    from dmesh_renderer_amd import _C
    m, B, H, W, rows = TET_CASES[case]
    dev = hip_device
    d = scenes.kuhn_tets(m, B, H, W)
    sc = oracle.scene_from_module_inputs(d, H, W, rows=rows)
    _, _, oactive, ost = oracle.tet_forward(sc)
    gc, gd, ga, gcd, gdad, gdd = _upstream(B, H, W, rows, dev)
    want_alpha = alpha_ref.expected_alpha(sc, ost, True, rows, oactive)
    og = oracle.tet_backward(sc, ost, gc.numpy(), gd.numpy())
    want_fo = og["faces_opacity"] + alpha_ref.alpha_opacity_grad(sc, ga.numpy(), True, rows)
    assert np.abs(want_fo - og["faces_opacity"]).max() > 1e-2, "the alpha term must matter"
    band = alpha_ref.band_mask(H, rows)[None, :, None] > 0
    inactive = (oactive < 0.5) & band
    assert 0.3 < inactive.sum() / band.sum() / (B * W) < 0.7, "the scene must have inactive pixels"
    g_inactive = th.cat([th.zeros(B, 1, H, W), th.from_numpy(inactive[:, None].astype(np.float32))], dim=1).to(dev)
    args = c_args(d, dev, tet=True)
    per_call = []
    for call in range(2):
        outa = _C.render_tets(*args, H, W, 0, rows=rows, alpha=True)
        gra = _np(_C.render_tets_backward(*args, gcd, gdad, *outa[3:7], rows=rows, alpha=True))
        th.cuda.synchronize()
        longest, cap = seq_state(_C, args, outa[3:7], H, W)
        assert (cap == 0) if call == 0 else (0 < longest <= cap), (call, longest, cap)
        gin = _np(_C.render_tets_backward(*args, th.zeros_like(gcd), g_inactive, *outa[3:7], rows=rows, alpha=True))
        gopt = {kw: _np(_C.render_tets_backward(*args, gcd, gdad, *outa[3:7], rows=rows, alpha=True, **{kw: True}))
                for kw in ("full_grads", "camera_grads")}
        # the calls without alpha: on the same forward state (the scratch buffers do not depend on the flag), so that both
        # run the same backward kernel -- a forward of its own would, in call 0, already have a march sequence
        gr0 = _np(_C.render_tets_backward(*args, gcd, gdd, *outa[3:7], rows=rows))
        gopt0 = {kw: _np(_C.render_tets_backward(*args, gcd, gdd, *outa[3:7], rows=rows, **{kw: True}))
                 for kw in ("full_grads", "camera_grads")}
        out0 = _C.render_tets(*args, H, W, 0, rows=rows)
        assert tuple(outa[1].shape) == (B, 2, H, W) and tuple(out0[1].shape) == (B, 1, H, W)
        assert th.equal(outa[0], out0[0]) and th.equal(outa[1][:, :1], out0[1]) and th.equal(outa[2], out0[2])
        assert np.array_equal(outa[2].cpu().numpy() * band, oactive * band)
        a = outa[1][:, 1].cpu().numpy()
        ea = float(np.abs(a[:, None] - want_alpha).max())
        ef = rel_err(gra[1], want_fo)
        print(f"\n{case} call {call}: alpha {ea:.2e}  dL_dfaces_opacity {ef:.2e}  (without the alpha term {rel_err(gr0[1], want_fo):.2e})")
        assert ea <= FWD_TOL and ef <= GRAD_TOL, (ea, ef)
        assert (a[oactive < 0.5] == 0).all() and (a[~np.broadcast_to(band, a.shape)] == 0).all()
        assert rel_err(gra[0], gr0[0]) <= SAME_TOL and rel_err(gra[0], og["verts_color"]) <= GRAD_TOL
        assert not np.abs(gin[0]).max() > 0 and not np.abs(gin[1]).max() > 0, "an inactive pixel's alpha has no gradient"
        for kw in gopt:  # -> (verts, verts_color, faces_opacity, faces_intense[, four matrices])
            assert len(gopt[kw]) == len(gopt0[kw])
            for i in range(len(gopt0[kw])):
                if i != 2:
                    assert rel_err(gopt[kw][i], gopt0[kw][i]) <= SAME_TOL, (kw, i)
            e = rel_err(gopt[kw][2], want_fo)
            print(f"{case} call {call} {kw}: dL_dfaces_opacity {e:.2e}")
            assert e <= GRAD_TOL, (kw, e)
        per_call.append(gra)
    for x, y in zip(*per_call):  # re-march vs sequence kernel
        assert rel_err(x, y) <= SAME_TOL


def test_modules_through_autograd(oracle, hip_device):
    """TriRenderer / TetRenderer(return_alpha=True): a loss on all outputs, and a mask loss on alpha alone."""
    import dmesh_renderer_amd as dmr
    dev = hip_device
    L, n, B, H, W, _ = TRI_CASES["two_views_ragged"]
    d = scenes.layered_sheets(L, n, B, H, W, seed=7, opacity=(0.1, 0.5))
    sc = oracle.scene_from_module_inputs(d, H, W)
    ocolor, _, ost = oracle.tri_forward(sc)
    gc, gd, ga, gcd, _, gdd = _upstream(B, H, W, (0, 0), dev)
    t = {k: v.to(dev) for k, v in d.items()}
    for loss in ("all", "alpha"):
        lv = {k: t[k].clone().requires_grad_(True) for k in TRI_NAMES}
        color, depth, alpha = dmr.TriRenderer(dmr.TriRenderSettings(H, W, t["bg"]), return_alpha=True)(
            lv["verts"], t["faces"], lv["verts_color"], lv["faces_opacity"], t["mv_mats"], t["proj_mats"], lv["verts_depth"], lv["faces_intense"])
        assert tuple(alpha.shape) == (B, 1, H, W) and tuple(depth.shape) == (B, 1, H, W)
        assert np.abs(alpha.detach().cpu().numpy() - alpha_ref.expected_alpha(sc, ost, False)).max() <= FWD_TOL
        if loss == "all":
            th.autograd.backward([color, depth, alpha], [gcd, gdd, ga.to(dev)])
            og = oracle.tri_backward(sc, ost, gc.numpy(), gd.numpy())
        else:
            (alpha * ga.to(dev)).sum().backward()
            og = {k: np.zeros_like(v) for k, v in oracle.tri_backward(sc, ost, gc.numpy(), gd.numpy()).items()}
        want = og["faces_opacity"] + alpha_ref.alpha_opacity_grad(sc, ga.numpy(), False)
        e = rel_err(lv["faces_opacity"].grad.cpu().numpy(), want)
        print(f"\ntri Module, loss on {loss}: dL_dfaces_opacity {e:.2e}")
        assert e <= GRAD_TOL
        for k in ("verts_color", "verts_depth", "faces_intense"):
            assert rel_err(lv[k].grad.cpu().numpy(), og[k]) <= GRAD_TOL, k
    # the background composited in torch: rendered over black, then + (1 - alpha) * bg
    black = dmr.TriRenderer(dmr.TriRenderSettings(H, W, th.zeros(3, device=dev)), return_alpha=True)
    c0, _, a0 = black(t["verts"], t["faces"], t["verts_color"], t["faces_opacity"], t["mv_mats"], t["proj_mats"], t["verts_depth"],
                      t["faces_intense"])
    over = c0 + (1 - a0) * t["bg"].view(1, 3, 1, 1)
    assert np.abs(over.cpu().numpy() - ocolor).max() <= FWD_TOL

    m, B, H, W, _ = TET_CASES["kuhn"]
    d = scenes.kuhn_tets(m, B, H, W)
    sc = oracle.scene_from_module_inputs(d, H, W)
    _, _, oactive, ost = oracle.tet_forward(sc)
    gc, gd, ga, gcd, _, gdd = _upstream(B, H, W, (0, 0), dev)
    t = {k: v.to(dev) for k, v in d.items()}
    (color, depth, active, alpha), g = module_step(dmr.TetRenderer(dmr.TetRenderSettings(H, W, t["bg"], 0), return_alpha=True), t,
                                                   ("verts_color", "faces_opacity"), [gcd, gdd, ga.to(dev)])
    assert active.dtype == th.bool and tuple(alpha.shape) == (B, 1, H, W)
    assert np.abs(alpha.cpu().numpy() - alpha_ref.expected_alpha(sc, ost, True, active=oactive)).max() <= FWD_TOL
    og = oracle.tet_backward(sc, ost, gc.numpy(), gd.numpy())
    e = rel_err(g["faces_opacity"].cpu().numpy(), og["faces_opacity"] + alpha_ref.alpha_opacity_grad(sc, ga.numpy(), True))
    print(f"tet Module, loss on all: dL_dfaces_opacity {e:.2e}")
    assert e <= GRAD_TOL and rel_err(g["verts_color"].cpu().numpy(), og["verts_color"]) <= GRAD_TOL


def test_binding_checks_the_two_channel_gradient(hip_device):
    from dmesh_renderer_amd import _C
    L, n, B, H, W, _ = TRI_CASES["one_view"]
    d = scenes.layered_sheets(L, n, B, H, W, seed=7)
    args = c_args(d, hip_device)
    gc, gd = upstream_grads(B, H, W)
    out = _C.render_tris(*args, H, W, alpha=True)
    with pytest.raises(RuntimeError, match=r"\(B, 2, H, W\)"):
        _C.render_tris_backward(*args, gc.to(hip_device), gd.to(hip_device), out[0], *out[3:7], alpha=True)


def test_alpha_step_replays_as_graph(hip_device):
    """One forward + backward with alpha captured with torch.cuda.graph matches the eager call."""
    from dmesh_renderer_amd import _C
    L, n, B, H, W, _ = TRI_CASES["two_views_ragged"]
    W = W + 16 * 11
    d = scenes.layered_sheets(L, n, B, H, W, seed=2)
    args = c_args(d, hip_device)
    _, _, _, gcd, gdad, _ = _upstream(B, H, W, (0, 0), hip_device)

    def step():
        out = _C.render_tris(*args, H, W, alpha=True)
        return (out[1], out[2]) + tuple(_C.render_tris_backward(*args, gcd, gdad, out[0], *out[3:7], alpha=True))

    graph, captured, eager = capture_replay(step)
    replay(graph)
    assert float(eager[1][:, 1].max()) > 0.3
    for a, b_ in zip(captured, eager):
        assert rel_err(a.cpu().numpy(), b_.cpu().numpy()) <= SAME_TOL


def test_two_ranks_alpha_match_single_rank(hip_device):
    """Sharded Modules with return_alpha=True, two ranks (gloo, one GPU), against the single-device Modules."""
    run_ranks("alpha", "sharded alpha ok")
