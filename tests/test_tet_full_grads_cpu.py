"""Full tet gradients (TetRenderer(full_grads=True): dL/dverts and dL/dfaces_intense, beyond the reference) -- the parts
that need no GPU: the float64 reference model of tests/tet_grad_ref.py pinned against the CPU oracle, the Python
plumbing with a stand-in `_C`, and the C ABI additions."""
import os
import re

import numpy as np
import pytest
import torch as th

import capi_ctypes
from dmesh_renderer_amd import scenes
from grad_cases import scene
from standins import _FakeC
from tet_grad_ref import TetGradRef
from util import rel_err, upstream_grads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = {  # name: (m, B, H, W, opacity, ray_random_seed) -- a smaller "small" than the GPU tests' (CPU time)
    "small": (4, 1, 64, 64, (0.02, 0.3), 0),
    "opaque": (6, 1, 64, 64, (0.6, 1.0), 0),
    "jitter": (4, 2, 48, 64, (0.05, 0.5), 7),
}


def _setup(oracle, case):
    d, B, H, W, seed = scene(case, cases=CASES)
    sc = oracle.scene_from_module_inputs(d, H, W, seed=seed)
    ocolor, odepth, _, ost = oracle.tet_forward(sc)
    return d, B, H, W, sc, ocolor, odepth, ost


@pytest.mark.parametrize("case", list(CASES))
def test_reference_model_matches_oracle(oracle, case):
    """The float64 brute-force model reproduces the oracle's forward on the kept pixels and its verts_color /
    faces_opacity gradients under the same masked upstream gradients: it is a model of the same renderer.
    One exception, "opaque" faces_opacity: faces of opacity ~0.99 there put the oracle's float32 `final_T / (1 - opacity)`
    and its remainder sums (backward.cu:290-330) 1.3e-3 (normalised) away from the float64 model; bound 2e-3."""
    d, B, H, W, sc, ocolor, odepth, ost = _setup(oracle, case)
    ref = TetGradRef(d, H, W, ost)
    assert ref.n_active > 100 and ref.kept_fraction >= 0.8, (ref.n_active, ref.kept_fraction)
    gc, gd = upstream_grads(B, H, W)
    m = ref.mask()
    gc, gd = gc * m, gd * m
    g, color, depth = ref.grads(gc, gd)
    HW = H * W
    b, r = ref.view.numpy(), (ref.pix % HW).numpy()
    oc = ocolor.reshape(B, 3, HW)[b, :, r]
    od = odepth.reshape(B, HW)[b, r]
    assert np.abs(color.numpy() - oc).max() <= 3e-5
    assert np.abs(depth.numpy() - od).max() <= 3e-5
    og = oracle.tet_backward(sc, ost, gc.numpy(), gd.numpy())
    for k in ("verts_color", "faces_opacity"):
        e = rel_err(g[k].astype(np.float32), og[k])
        assert e <= (2e-3 if (case, k) == ("opaque", "faces_opacity") else 1e-4), (k, e)
    assert np.abs(g["verts"]).max() > 0 and np.abs(g["faces_intense"]).max() > 0


@pytest.mark.parametrize("full", [False, True])
def test_module_routes_full_grads(monkeypatch, full):
    import dmesh_renderer_amd as dmr
    fake = _FakeC()
    monkeypatch.setattr(dmr._C, "render_tets", fake.render_tets)
    monkeypatch.setattr(dmr._C, "render_tets_backward", fake.render_tets_backward)
    B, H, W = 2, 32, 48
    d = scenes.kuhn_tets(2, B, H, W)
    leaves = {k: d[k].clone().requires_grad_(True) for k in ("verts", "verts_color", "faces_opacity", "verts_depth", "faces_intense")}
    r = dmr.TetRenderer(dmr.TetRenderSettings(H, W, d["bg"], 0), full_grads=full) if full else \
        dmr.TetRenderer(dmr.TetRenderSettings(H, W, d["bg"], 0))
    color, depth, _ = r(leaves["verts"], d["faces"], leaves["verts_color"], leaves["faces_opacity"], d["mv_mats"],
                        d["proj_mats"], leaves["verts_depth"], leaves["faces_intense"], d["tets"], d["face_tets"], d["tet_faces"])
    (color.sum() + depth.sum()).backward()
    assert len(fake.calls) == 1
    nargs, kw = fake.calls[0]
    assert nargs == 20
    assert leaves["verts_color"].grad is not None and th.all(leaves["verts_color"].grad == 2.0)
    assert th.all(leaves["faces_opacity"].grad == 3.0)
    assert leaves["verts_depth"].grad is None
    if full:
        assert kw == {"rows": (0, 0), "full_grads": True}
        assert th.all(leaves["verts"].grad == 1.0) and th.all(leaves["faces_intense"].grad == 4.0)
    else:  # the reference's call: no new keyword, no new gradient
        assert kw == {"rows": (0, 0)}
        assert leaves["verts"].grad is None and leaves["faces_intense"].grad is None


def test_sharded_module_routes_full_grads():
    """ShardedTetRenderer(full_grads=True) on one rank through an impl without flat_out support."""
    from dmesh_renderer_amd import TetRenderSettings, sharding
    fake = _FakeC()
    B, H, W = 1, 32, 32
    d = scenes.kuhn_tets(2, B, H, W)
    for full in (False, True):
        fake.calls.clear()
        sh = sharding.ShardedTetRenderer(TetRenderSettings(H, W, d["bg"], 0), impl=fake, full_grads=full)
        v = d["verts"].clone().requires_grad_(True); fi = d["faces_intense"].clone().requires_grad_(True)
        c, z, _ = sh(v, d["faces"], d["verts_color"], d["faces_opacity"], d["mv_mats"], d["proj_mats"], d["verts_depth"], fi,
                     d["tets"], d["face_tets"], d["tet_faces"])
        (c.sum() + z.sum()).backward()
        assert fake.calls[0][1].get("full_grads", False) == full
        assert (v.grad is not None) == full and (fi.grad is not None) == full
        if full:
            assert th.all(v.grad == 1.0) and th.all(fi.grad == 4.0)


def test_header_declares_flag_and_buffer():
    with open(os.path.join(ROOT, "include", "dmesh_renderer_amd.h")) as f:
        src = f.read()
    assert re.search(r"#define\s+DMR_FLAG_TET_FULL_GRADS\s+2\b", src)
    assert re.search(r"\bDMR_BUF_TET_GRADS\s*=\s*5\b", src)
    assert re.search(r"#define\s+DMR_ABI_VERSION\s+4\b", src)
    declared = set(re.findall(r"\b(dmr_[a-z_0-9]+)\s*\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S)))
    assert declared <= set(capi_ctypes.EXPORTS), declared - set(capi_ctypes.EXPORTS)
