"""The alpha (coverage) output without a GPU: the C header's flag, the binding's keyword, and the Python plumbing of
TriRenderer / TetRenderer / the sharded Modules (return_alpha=True) over the oracle-backed stand-in of tests/alpha_ref.py.

Expected values come from the CPU oracle by the two identities of tests/alpha_ref.py; bounds are the project's own
(forward 1e-5 absolute, gradients rel_err <= 1e-4, "same as the default path" 1e-5)."""
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch as th
import torch.distributed as dist
import torch.multiprocessing as mp

import alpha_ref
import oracle_C
from dmesh_renderer_amd import scenes
from harness import free_port
from util import rel_err, upstream_grads

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FWD_TOL, GRAD_TOL, SAME_TOL = 1e-5, 1e-4, 1e-5

TRI = dict(L=3, n=6, B=2, H=40, W=56, seed=4)   # the scenes of tests/test_wrapper_cpu.py
TET = dict(m=3, B=2, H=48, W=48, seed=2)
TRI_LEAVES = ("verts", "verts_color", "faces_opacity", "verts_depth", "faces_intense")


def _alpha_upstream(B, H, W):
    return th.randn(B, 1, H, W, generator=th.Generator().manual_seed(5))


def test_header_flag_and_abi_version():
    h = open(os.path.join(ROOT, "include", "dmesh_renderer_amd.h")).read()
    assert re.search(r"#define DMR_FLAG_ALPHA 32\b", h)
    assert re.search(r"#define DMR_ABI_VERSION 4\b", h)
    from dmesh_renderer_amd import _C
    assert _C.ABI_VERSION == 4


@pytest.mark.parametrize("fn", ["render_tris", "render_tris_backward", "render_tets", "render_tets_backward"])
def test_binding_accepts_alpha_keyword(fn):
    from dmesh_renderer_amd import _C
    doc = getattr(_C, fn).__doc__
    assert re.search(r"\*, .*alpha: bool = False", doc), doc  # keyword-only, off by default


@pytest.fixture()
def ours(monkeypatch, oracle):
    import dmesh_renderer_amd as dmr
    for n in ("render_tris", "render_tris_backward", "render_tets", "render_tets_backward"):
        monkeypatch.setattr(dmr._C, n, getattr(alpha_ref, n))
    oracle_C.calls.clear()
    alpha_ref.kwargs_seen.clear()
    return dmr


def _tri_leaves(d):
    return {k: d[k].clone().requires_grad_(True) for k in TRI_LEAVES}


def _tri_call(r, d, lv):
    return r(lv["verts"], d["faces"].long(), lv["verts_color"], lv["faces_opacity"], d["mv_mats"], d["proj_mats"],
             lv["verts_depth"], lv["faces_intense"])


def _tet_call(r, d, vc, fo):
    return r(d["verts"], d["faces"].long(), vc, fo, d["mv_mats"], d["proj_mats"], d["verts_depth"], d["faces_intense"],
             d["tets"].long(), d["face_tets"].long(), d["tet_faces"].long())


@pytest.mark.parametrize("loss", ["alpha", "color", "all"])
def test_tri_module_returns_alpha_and_routes_its_gradient(ours, oracle, loss):
    B, H, W = TRI["B"], TRI["H"], TRI["W"]
    d = scenes.layered_sheets(TRI["L"], TRI["n"], B, H, W, seed=TRI["seed"])
    sc = oracle.scene_from_module_inputs(d, H, W)
    ocolor, odepth, ost = oracle.tri_forward(sc)
    lv = _tri_leaves(d)
    out = _tri_call(ours.TriRenderer(ours.TriRenderSettings(H, W, d["bg"]), return_alpha=True), d, lv)
    assert len(out) == 3
    color, depth, alpha = out
    assert tuple(alpha.shape) == (B, 1, H, W) and tuple(depth.shape) == (B, 1, H, W)
    assert th.equal(color.detach(), th.from_numpy(ocolor)) and th.equal(depth.detach(), th.from_numpy(odepth))
    want = alpha_ref.expected_alpha(sc, ost, False)
    assert np.abs(alpha.detach().numpy() - want).max() <= FWD_TOL
    assert want.max() > 0.3 and want.min() == 0.0, "the scene must have covered and empty pixels"
    # color == C + (1 - alpha) * bg: with the twin's background T itself is visible
    gc, gd = upstream_grads(B, H, W)
    ga = _alpha_upstream(B, H, W)
    z = lambda t: th.zeros_like(t)
    gc, gd, ga = {"alpha": (z(gc), z(gd), ga), "color": (gc, z(gd), z(ga)), "all": (gc, gd, ga)}[loss]
    {"alpha": lambda: (alpha * ga).sum(), "color": lambda: (color * gc).sum(),
     "all": lambda: (color * gc).sum() + (depth * gd).sum() + (alpha * ga).sum()}[loss]().backward()
    og = oracle.tri_backward(sc, ost, gc.numpy(), gd.numpy())
    og["faces_opacity"] = og["faces_opacity"] + alpha_ref.alpha_opacity_grad(sc, ga.numpy(), False)
    for k in TRI_LEAVES:
        e = rel_err(lv[k].grad.numpy(), og[k])
        print(f"tri {loss} {k}: {e:.2e}")
        assert e <= (GRAD_TOL if k == "faces_opacity" else SAME_TOL), (k, e)
    if loss == "alpha":
        assert np.abs(og["faces_opacity"]).max() > 1e-2
        for k in TRI_LEAVES:
            if k != "faces_opacity":
                assert not lv[k].grad.abs().max() > 0, k
    assert alpha_ref.kwargs_seen == [("render_tris", ["alpha"]), ("render_tris_backward", ["alpha"])]


@pytest.mark.parametrize("loss", ["alpha", "color", "all"])
def test_tet_module_returns_alpha_and_routes_its_gradient(ours, oracle, loss):
    B, H, W = TET["B"], TET["H"], TET["W"]
    d = scenes.kuhn_tets(TET["m"], B, H, W, seed=TET["seed"])
    sc = oracle.scene_from_module_inputs(d, H, W)
    ocolor, odepth, oactive, ost = oracle.tet_forward(sc)
    vc, fo = d["verts_color"].clone().requires_grad_(True), d["faces_opacity"].clone().requires_grad_(True)
    out = _tet_call(ours.TetRenderer(ours.TetRenderSettings(H, W, d["bg"], 0), return_alpha=True), d, vc, fo)
    assert len(out) == 4
    color, depth, active, alpha = out
    assert active.dtype == th.bool and tuple(alpha.shape) == (B, 1, H, W) and tuple(depth.shape) == (B, 1, H, W)
    assert th.equal(color.detach(), th.from_numpy(ocolor)) and th.equal(depth.detach(), th.from_numpy(odepth))
    want = alpha_ref.expected_alpha(sc, ost, True, active=oactive)
    assert np.abs(alpha.detach().numpy() - want).max() <= FWD_TOL
    assert 0.1 < oactive.mean() < 0.9
    assert (alpha.detach().numpy()[:, 0][oactive < 0.5] == 0).all(), "alpha is exactly 0 where the march fails"
    gc, gd = upstream_grads(B, H, W)
    ga = _alpha_upstream(B, H, W)
    z = lambda t: th.zeros_like(t)
    gc, gd, ga = {"alpha": (z(gc), z(gd), ga), "color": (gc, z(gd), z(ga)), "all": (gc, gd, ga)}[loss]
    {"alpha": lambda: (alpha * ga).sum(), "color": lambda: (color * gc).sum(),
     "all": lambda: (color * gc).sum() + (depth * gd).sum() + (alpha * ga).sum()}[loss]().backward()
    og = oracle.tet_backward(sc, ost, gc.numpy(), gd.numpy())
    want_fo = og["faces_opacity"] + alpha_ref.alpha_opacity_grad(sc, ga.numpy(), True)
    e = rel_err(fo.grad.numpy(), want_fo)
    print(f"tet {loss} faces_opacity: {e:.2e}")
    assert e <= GRAD_TOL
    assert rel_err(vc.grad.numpy(), og["verts_color"]) <= SAME_TOL
    if loss == "alpha":
        assert np.abs(want_fo).max() > 1e-2 and not vc.grad.abs().max() > 0
    assert alpha_ref.kwargs_seen == [("render_tets", ["alpha"]), ("render_tets_backward", ["alpha"])]


def test_functional_forms_return_alpha_last(ours, oracle):
    B, H, W = TRI["B"], TRI["H"], TRI["W"]
    d = scenes.layered_sheets(TRI["L"], TRI["n"], B, H, W, seed=TRI["seed"])
    mv, pr = d["mv_mats"].transpose(1, 2), d["proj_mats"].transpose(1, 2)
    st = ours.TriRenderSettings(H, W, d["bg"])
    a = (d["verts"], d["faces"], d["verts_color"], d["faces_opacity"], mv, pr, d["verts_depth"], d["faces_intense"], st)
    c3 = ours.render_tri(*a, return_alpha=True)
    c2 = ours.render_tri(*a)
    assert len(c3) == 3 and len(c2) == 2 and th.equal(c3[0], c2[0]) and th.equal(c3[1], c2[1])
    d = scenes.kuhn_tets(TET["m"], TET["B"], TET["H"], TET["W"], seed=TET["seed"])
    mv, pr = d["mv_mats"].transpose(1, 2), d["proj_mats"].transpose(1, 2)
    st = ours.TetRenderSettings(TET["H"], TET["W"], d["bg"], 0)
    a = (d["verts"], d["faces"], d["verts_color"], d["faces_opacity"], mv, pr, d["verts_depth"], d["faces_intense"],
         d["tets"], d["face_tets"], d["tet_faces"], st)
    c4 = ours.render_tet(*a, return_alpha=True)
    c3 = ours.render_tet(*a)
    assert len(c4) == 4 and len(c3) == 3 and c4[2].dtype == th.bool and tuple(c4[3].shape) == (TET["B"], 1, TET["H"], TET["W"])


def test_default_modules_make_the_calls_they_made(ours):
    """Without return_alpha: no `alpha` keyword reaches `_C`, the argument descriptors are the golden ones, two / three
    outputs, and the Functions' apply takes its ten / thirteen arguments."""
    with open(os.path.join(HERE, "golden", "wrapper_calls.json")) as f:
        gold = json.load(f)
    B, H, W = TRI["B"], TRI["H"], TRI["W"]
    d = scenes.layered_sheets(TRI["L"], TRI["n"], B, H, W, seed=TRI["seed"])
    gc, gd = upstream_grads(B, H, W)
    lv = _tri_leaves(d)
    r = ours.TriRenderer(ours.TriRenderSettings(H, W, d["bg"]))
    assert r.return_alpha is False
    out = _tri_call(r, d, lv)
    assert len(out) == 2
    ((out[0] * gc).sum() + (out[1] * gd).sum()).backward()
    assert alpha_ref.kwargs_seen == [("render_tris", []), ("render_tris_backward", [])]
    assert json.loads(json.dumps(oracle_C.calls)) == gold["tri"]
    oracle_C.calls.clear(); alpha_ref.kwargs_seen.clear()
    B, H, W = TET["B"], TET["H"], TET["W"]
    d = scenes.kuhn_tets(TET["m"], B, H, W, seed=TET["seed"])
    gc, gd = upstream_grads(B, H, W)
    vc, fo = d["verts_color"].clone().requires_grad_(True), d["faces_opacity"].clone().requires_grad_(True)
    out = ours.TetRenderer(ours.TetRenderSettings(H, W, d["bg"], 0))(
        d["verts"].double(), d["faces"].long(), vc, fo, d["mv_mats"].double(), d["proj_mats"], d["verts_depth"], d["faces_intense"],
        d["tets"].long(), d["face_tets"].long(), d["tet_faces"].long())
    assert len(out) == 3
    ((out[0] * gc).sum() + (out[1] * gd).sum()).backward()
    assert alpha_ref.kwargs_seen == [("render_tets", []), ("render_tets_backward", [])]
    assert json.loads(json.dumps(oracle_C.calls)) == gold["tet"]
    import dmesh_renderer_amd as dmr
    assert dmr._trailing(None, False, False, False) == ()
    assert "alpha" in inspect.signature(dmr._TriFn.forward).parameters and "alpha" in inspect.signature(dmr._TetFn.forward).parameters


# ---- gloo, world size 2, both partitions -----------------------------------------------------------------------------
def _sharded_scene():
    H, W, B = 88, 72, 2
    return scenes.layered_sheets(3, 7, B, H, W, seed=1), scenes.kuhn_tets(3, B, H, W, seed=2), B, H, W


def _run_tri(r, d, gc, gd, ga):
    lv = _tri_leaves(d)
    color, depth, alpha = _tri_call(r, d, lv)
    ((color * gc).sum() + (depth * gd).sum() + (alpha * ga).sum()).backward()
    return [color.detach(), depth.detach(), alpha.detach()] + [lv[k].grad for k in TRI_LEAVES]


def _run_tet(r, d, gc, gd, ga):
    vc, fo = d["verts_color"].clone().requires_grad_(True), d["faces_opacity"].clone().requires_grad_(True)
    color, depth, active, alpha = _tet_call(r, d, vc, fo)
    ((color * gc).sum() + (depth * gd).sum() + (alpha * ga).sum()).backward()
    return [color.detach(), depth.detach(), active.float(), alpha.detach(), vc.grad, fo.grad]


def _worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    os.environ["OMP_NUM_THREADS"] = "2"
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import dmesh_renderer_amd as dmr
        from dmesh_renderer_amd import sharding
        import alpha_ref as A
        tri, tet, B, H, W = _sharded_scene()
        gc, gd = upstream_grads(B, H, W)
        ga = _alpha_upstream(B, H, W)
        res = {}
        for partition in ("bands", "view_bands"):
            r = sharding.ShardedTriRenderer(dmr.TriRenderSettings(H, W, tri["bg"]), assemble=True, impl=A, partition=partition,
                                            return_alpha=True)
            assert r.world == 2 and r._use_view_bands(B) == (partition == "view_bands")
            for i, t in enumerate(_run_tri(r, tri, gc, gd, ga)):
                res[f"tri_{partition}_{i}"] = t.numpy()
        r = sharding.ShardedTetRenderer(dmr.TetRenderSettings(H, W, tet["bg"], 0), assemble=True, impl=A, return_alpha=True)
        for i, t in enumerate(_run_tet(r, tet, gc, gd, ga)):
            res[f"tet_{i}"] = t.numpy()
        np.savez(os.path.join(out_dir, f"alpha{rank}.npz"), **res)
    finally:
        dist.destroy_process_group()


def test_two_rank_sharded_alpha_equals_single_rank(tmp_path, ours):
    """ShardedTriRenderer (both partitions) and ShardedTetRenderer with return_alpha=True on two gloo ranks: every rank
    ends with the images and gradients of the single-rank Module."""
    mp.spawn(_worker, args=(2, free_port(), str(tmp_path)), nprocs=2, join=True)
    tri, tet, B, H, W = _sharded_scene()
    gc, gd = upstream_grads(B, H, W)
    ga = _alpha_upstream(B, H, W)
    full_tri = _run_tri(ours.TriRenderer(ours.TriRenderSettings(H, W, tri["bg"]), return_alpha=True), tri, gc, gd, ga)
    full_tet = _run_tet(ours.TetRenderer(ours.TetRenderSettings(H, W, tet["bg"], 0), return_alpha=True), tet, gc, gd, ga)
    assert full_tri[2].max() > 0.3 and full_tet[3].max() > 0.1
    for rank in range(2):
        r = np.load(tmp_path / f"alpha{rank}.npz")
        for partition in ("bands", "view_bands"):
            for i, t in enumerate(full_tri):
                got = r[f"tri_{partition}_{i}"]
                if i < 3:
                    assert np.array_equal(got, t.numpy()), (partition, i)
                else:
                    assert rel_err(got, t.numpy()) <= SAME_TOL, (partition, i)
        for i, t in enumerate(full_tet):
            got = r[f"tet_{i}"]
            if i < 4:
                assert np.array_equal(got, t.numpy()), i
            else:
                assert rel_err(got, t.numpy()) <= SAME_TOL, i
