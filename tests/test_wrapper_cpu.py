"""Host-side mirror of the reference interface, checked on CPU with the oracle-backed `_C` stand-in:
  * our wrapper (dmesh_renderer_amd) routes arguments / gradients like the reference wrapper,
  * the REFERENCE wrapper's own run over the same stand-in is stored in tests/golden (outputs and gradients in
    wrapper_*.npz, the argument descriptors of each of its `_C` calls in wrapper_calls.json, all written by
    tests/golden/gen_wrapper_fixtures.py from a reference checkout): ours must agree with it exactly -- that is
    the drop-in proof for the Python boundary,
  * ours must reproduce the golden fixtures.
"""
import json
import os

import numpy as np
import pytest
import torch as th

import oracle_C
from dmesh_renderer_amd import scenes
from util import upstream_grads

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture()
def ours(monkeypatch, oracle):
    import dmesh_renderer_amd as dmr
    for n in ("render_tris", "render_tris_backward", "render_tets", "render_tets_backward"):
        monkeypatch.setattr(dmr._C, n, getattr(oracle_C, n))
    oracle_C.calls.clear()
    return dmr


def jsonable(calls):
    """oracle_C.calls as stored in tests/golden/wrapper_calls.json (tuples become lists)."""
    return json.loads(json.dumps(calls))


def _reference_run(kind):
    """What the reference wrapper returned and passed to `_C` on the scene of `kind` (tests/golden/gen_wrapper_fixtures.py)."""
    g = np.load(os.path.join(GOLD, f"wrapper_{kind}.npz"))
    with open(os.path.join(GOLD, "wrapper_calls.json")) as f:
        calls = json.load(f)[kind]
    return {k: th.from_numpy(g[k]) for k in g.files}, calls


def _tri_run(mod, d, H, W):
    leaves = {k: d[k].clone().requires_grad_(True) for k in ("verts", "verts_color", "faces_opacity", "verts_depth", "faces_intense")}
    r = mod.TriRenderer(mod.TriRenderSettings(H, W, d["bg"]))
    color, depth = r(leaves["verts"], d["faces"].long(), leaves["verts_color"], leaves["faces_opacity"],
                     d["mv_mats"], d["proj_mats"], leaves["verts_depth"], leaves["faces_intense"])
    gc, gd = upstream_grads(d["mv_mats"].shape[0], H, W)
    # a non-contiguous incoming gradient, as autograd delivers for sums
    ((color * gc).sum() + (depth * gd).sum()).backward()
    return color.detach(), depth.detach(), {k: v.grad for k, v in leaves.items()}


def _tet_run(mod, d, H, W):
    vc = d["verts_color"].clone().requires_grad_(True); fo = d["faces_opacity"].clone().requires_grad_(True)
    r = mod.TetRenderer(mod.TetRenderSettings(H, W, d["bg"], 0))
    color, depth, active = r(d["verts"].double(), d["faces"].long(), vc, fo, d["mv_mats"].double(), d["proj_mats"],
                             d["verts_depth"], d["faces_intense"], d["tets"].long(), d["face_tets"].long(), d["tet_faces"].long())
    gc, gd = upstream_grads(d["mv_mats"].shape[0], H, W)
    ((color * gc).sum() + (depth * gd).sum()).backward()
    return color.detach(), depth.detach(), active, {"verts_color": vc.grad, "faces_opacity": fo.grad}


TRI = dict(L=3, n=6, B=2, H=40, W=56, seed=4)
TET = dict(m=3, B=2, H=48, W=48, seed=2)


def _tri_scene():
    return scenes.layered_sheets(TRI["L"], TRI["n"], TRI["B"], TRI["H"], TRI["W"], seed=TRI["seed"])


def _tet_scene():
    return scenes.kuhn_tets(TET["m"], TET["B"], TET["H"], TET["W"], seed=TET["seed"])


def test_tri_call_protocol(ours):
    d = _tri_scene()
    color, depth, grads = _tri_run(ours, d, TRI["H"], TRI["W"])
    (n1, a1), (n2, a2) = oracle_C.calls
    assert n1 == "render_tris" and len(a1) == 13 and n2 == "render_tris_backward" and len(a2) == 18
    # mats arrive as transposed views (stride (16,1,4)), faces as int32 (reference __init__.py:215-220)
    assert a1[5][3] == (16, 1, 4) and a1[6][3] == (16, 1, 4) and a1[2][1] == "torch.int32"
    assert tuple(color.shape) == (TRI["B"], 3, TRI["H"], TRI["W"]) and tuple(depth.shape) == (TRI["B"], 1, TRI["H"], TRI["W"])
    assert all(g is not None and g.shape == d[k].shape for k, g in grads.items())


def test_tet_call_protocol(ours):
    d = _tet_scene()
    color, depth, active, grads = _tet_run(ours, d, TET["H"], TET["W"])
    (n1, a1), (n2, a2) = oracle_C.calls
    assert n1 == "render_tets" and len(a1) == 17 and n2 == "render_tets_backward" and len(a2) == 20
    assert a1[1][1] == "torch.float32" and a1[11][1] == "torch.int32"  # the tet Module casts everything (Q23)
    assert active.dtype == th.bool and tuple(active.shape) == (TET["B"], TET["H"], TET["W"])


def test_tri_matches_reference_wrapper(ours):
    ref, ref_calls = _reference_run("tri")
    oc, od, og = _tri_run(ours, _tri_scene(), TRI["H"], TRI["W"])
    assert th.equal(oc, ref["color"]) and th.equal(od, ref["depth"])
    assert sorted("grad_" + k for k in og) == sorted(k for k in ref if k.startswith("grad_"))
    for k in og:
        assert th.equal(og[k], ref["grad_" + k]), k
    assert jsonable(oracle_C.calls) == ref_calls  # identical argument descriptors (order, dtype, shape, stride)


def test_tet_matches_reference_wrapper(ours):
    ref, ref_calls = _reference_run("tet")
    oc, od, oa, og = _tet_run(ours, _tet_scene(), TET["H"], TET["W"])
    assert th.equal(oc, ref["color"]) and th.equal(od, ref["depth"]) and th.equal(oa, ref["active"])
    assert sorted("grad_" + k for k in og) == sorted(k for k in ref if k.startswith("grad_"))
    for k in og:
        assert th.equal(og[k], ref["grad_" + k]), k
    assert jsonable(oracle_C.calls) == ref_calls


def test_golden_fixtures(ours):
    """Fixtures were produced by the REFERENCE wrapper over the oracle stand-in; our wrapper must reproduce them."""
    g = np.load(os.path.join(GOLD, "wrapper_tri.npz"))
    oc, od, og = _tri_run(ours, _tri_scene(), TRI["H"], TRI["W"])
    np.testing.assert_array_equal(oc.numpy(), g["color"]); np.testing.assert_array_equal(od.numpy(), g["depth"])
    for k in og:
        np.testing.assert_allclose(og[k].numpy(), g["grad_" + k], rtol=0, atol=1e-6 * max(1.0, np.abs(g["grad_" + k]).max()))
    g = np.load(os.path.join(GOLD, "wrapper_tet.npz"))
    oc, od, oa, og = _tet_run(ours, _tet_scene(), TET["H"], TET["W"])
    np.testing.assert_array_equal(oc.numpy(), g["color"]); np.testing.assert_array_equal(oa.numpy(), g["active"])
    for k in og:
        np.testing.assert_allclose(og[k].numpy(), g["grad_" + k], rtol=0, atol=1e-6 * max(1.0, np.abs(g["grad_" + k]).max()))
