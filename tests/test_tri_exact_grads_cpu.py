"""The float64 model of tests/tri_grad_ref.py pinned to the CPU oracle, and the Python plumbing of the tri gradient options
(TriRenderer(exact_grads=..., camera_grads=...)) over a stand-in `_C`.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch as th

from dmesh_renderer_amd import scenes
from standins import _StandIn
from tri_grad_ref import TriGradRef
from util import rel_err, upstream_grads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pinned(oracle):
    B, H, W = 2, 48, 80
    d = scenes.layered_sheets(3, 7, B, H, W, seed=3)
    sc = oracle.scene_from_module_inputs(d, H, W)
    _, _, ost = color_depth_state = oracle.tri_forward(sc)
    ref = TriGradRef(d, H, W, ost)
    return d, B, H, W, sc, color_depth_state, ref


def test_model_rays_match_oracle(pinned):
    d, B, H, W, sc, (_, _, ost), ref = pinned
    ro = ost.get("ray_o").reshape(B, H, W, 3)
    rd = ost.get("ray_d").reshape(B, H, W, 3)
    assert np.abs(ref.ray_o.numpy() - ro).max() <= 2e-6 * max(1.0, np.abs(ro).max())
    assert np.abs(ref.ray_d.numpy() - rd).max() <= 2e-6


def test_model_forward_matches_oracle(pinned):
    d, B, H, W, sc, (color, depth, _), ref = pinned
    assert ref.kept_fraction >= 0.8, ref.kept_fraction
    assert ref.faces_of.shape[0] > 100
    leaves = {k: d[k].to(th.float64) for k in ("verts", "verts_color", "faces_opacity", "verts_depth", "faces_intense",
                                                "mv_mats", "proj_mats")}
    with th.no_grad():
        c, z = ref.render(leaves)
    oc = color[ref.view.numpy(), :, ref.py.numpy(), ref.px.numpy()]
    oz = depth[ref.view.numpy(), 0, ref.py.numpy(), ref.px.numpy()]
    assert np.abs(c.numpy() - oc).max() <= 1e-5
    assert np.abs(z.numpy() - oz).max() <= 1e-5


def test_model_default_gradients_match_oracle(oracle, pinned):
    """The four gradients the reference computes exactly (all but verts) agree with the oracle's tri_backward."""
    d, B, H, W, sc, (_, _, ost), ref = pinned
    gc, gd = upstream_grads(B, H, W)
    m = ref.mask()
    gc, gd = gc * m, gd * m
    g, _, _ = ref.grads(gc, gd)
    og = oracle.tri_backward(sc, ost, gc.numpy(), gd.numpy())
    for k in ("verts_color", "faces_opacity", "verts_depth", "faces_intense"):
        assert rel_err(og[k], g[k]) <= 1e-4, k
    # the reference's dL_dverts is not the derivative: the model must disagree with it
    assert rel_err(og["verts"], g["verts"]) > 1e-2


@pytest.mark.parametrize("opts", [{}, {"exact_grads": True}, {"camera_grads": True}, {"exact_grads": True, "camera_grads": True}])
def test_plumbing_keywords_and_inverse_chain_rule(monkeypatch, opts):
    import dmesh_renderer_amd as dmr
    B, P, F, H, W = 2, 4, 2, 8, 8
    gen = th.Generator().manual_seed(0)
    g_inv = (th.randn(B, 4, 4, generator=gen, dtype=th.float64), th.randn(B, 4, 4, generator=gen, dtype=th.float64))
    fake = _StandIn(B, P, F, H, W, g_inv)
    monkeypatch.setattr(dmr, "_C", fake)
    mv = (th.eye(4, dtype=th.float64) + 0.1 * th.randn(B, 4, 4, generator=gen, dtype=th.float64)).requires_grad_(True)
    proj = (th.eye(4, dtype=th.float64) + 0.1 * th.randn(B, 4, 4, generator=gen, dtype=th.float64)).requires_grad_(True)
    verts = th.zeros(P, 3, dtype=th.float64, requires_grad=True)
    r = dmr.TriRenderer(dmr.TriRenderSettings(H, W, th.zeros(3)), **opts)
    color, depth = r(verts, th.zeros(F, 3, dtype=th.int32), th.zeros(P, 3, dtype=th.float64), th.zeros(F, dtype=th.float64),
                     mv, proj, th.zeros(B, P, dtype=th.float64), th.zeros(B, F, dtype=th.float64))
    (color.sum() + depth.sum()).backward()
    want = {"camera_grads": True} if opts.get("camera_grads") else ({"exact_grads": True} if opts else {})
    assert fake.kw == [want]
    if not opts.get("camera_grads"):
        assert mv.grad is None and proj.grad is None
        return
    # the Functions receive mv^T, proj^T; the kernels' gradients are those of inverse(mv^T), inverse(proj^T)
    m2, p2 = mv.detach().clone().requires_grad_(True), proj.detach().clone().requires_grad_(True)
    ((th.inverse(m2.transpose(1, 2)) * g_inv[0]).sum() + (th.inverse(p2.transpose(1, 2)) * g_inv[1]).sum()).backward()
    assert th.allclose(mv.grad, m2.grad, rtol=1e-12, atol=1e-12)
    assert th.allclose(proj.grad, p2.grad, rtol=1e-12, atol=1e-12)


def test_camera_grads_only_when_a_matrix_asks(monkeypatch):
    """camera_grads with matrices that need no gradient: the exact variant is called, the matrices get None."""
    import dmesh_renderer_amd as dmr
    B, P, F, H, W = 1, 3, 1, 8, 8
    fake = _StandIn(B, P, F, H, W, ())
    monkeypatch.setattr(dmr, "_C", fake)
    verts = th.zeros(P, 3, dtype=th.float64, requires_grad=True)
    eye = th.eye(4, dtype=th.float64)[None]
    color, _ = dmr.render_tri(verts, th.zeros(F, 3, dtype=th.int32), th.zeros(P, 3, dtype=th.float64), th.zeros(F, dtype=th.float64),
                              eye, eye, th.zeros(B, P, dtype=th.float64), th.zeros(B, F, dtype=th.float64),
                              dmr.TriRenderSettings(H, W, th.zeros(3)), camera_grads=True)
    color.sum().backward()
    assert fake.kw == [{"exact_grads": True}]


def test_header_constants():
    h = open(os.path.join(ROOT, "include", "dmesh_renderer_amd.h")).read()
    assert re.search(r"#define DMR_FLAG_TRI_EXACT_GRADS 4\b", h)
    assert re.search(r"#define DMR_FLAG_TRI_CAMERA_GRADS 8\b", h)
    assert re.search(r"DMR_BUF_TRI_CAMERA_GRADS = 6\b", h)
    assert re.search(r"#define DMR_ABI_VERSION 4\b", h)
