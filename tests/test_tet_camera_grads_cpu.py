"""Tet camera gradients (TetRenderer(camera_grads=True): dL/dmv_mats and dL/dproj_mats, beyond the reference) -- the parts
that need no GPU: the float64 model of tests/tet_camera_grad_ref.py pinned to the CPU oracle and to its own central
differences, the Python plumbing with a stand-in `_C`, and the C ABI additions."""
import os
import re

import numpy as np
import pytest
import torch as th

from dmesh_renderer_amd import scenes
from grad_cases import scene
from harness import free_port
from standins import _FakeC
from tet_camera_grad_ref import TetCameraGradRef
from util import rel_err, upstream_grads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = {  # name: (m, B, H, W, opacity, ray_random_seed)
    "small": (3, 1, 48, 48, (0.02, 0.3), 0),
    "opaque": (4, 1, 48, 48, (0.6, 1.0), 0),
    "jitter": (3, 2, 32, 48, (0.05, 0.5), 7),
}


def _setup(oracle, case):
    d, B, H, W, seed = scene(case, cases=CASES)
    sc = oracle.scene_from_module_inputs(d, H, W, seed=seed)
    ocolor, odepth, _, ost = oracle.tet_forward(sc)
    ref = TetCameraGradRef(d, H, W, ost, seed=seed)
    gc, gd = upstream_grads(B, H, W)
    m = ref.mask()
    return d, B, H, W, ocolor, odepth, ref, gc * m, gd * m


@pytest.mark.parametrize("case", list(CASES))
def test_model_forward_matches_oracle(oracle, case):
    """The rays rebuilt from the float64 matrices give the oracle's colour and depth on the kept pixels."""
    d, B, H, W, ocolor, odepth, ref, gc, gd = _setup(oracle, case)
    assert ref.n_active > 100 and ref.kept_fraction >= 0.8, (ref.n_active, ref.kept_fraction)
    with th.no_grad():
        color, depth = ref.render(ref.leaves())
    HW = H * W
    b, r = ref.view.numpy(), (ref.pix % HW).numpy()
    assert np.abs(color.numpy() - ocolor.reshape(B, 3, HW)[b, :, r]).max() <= 3e-5
    assert np.abs(depth.numpy() - odepth.reshape(B, HW)[b, r]).max() <= 3e-5
    o, dr = ref.rays(ref.d["mv_mats"].to(th.float64), ref.d["proj_mats"].to(th.float64))
    assert (o - ref.ro).abs().max() <= 1e-5 and (dr - ref.rd).abs().max() <= 1e-5


@pytest.mark.parametrize("case", list(CASES))
def test_model_matrix_grads_match_central_differences(oracle, case):
    """Autograd of the float64 model against its own central differences, every entry of both matrices of every view."""
    d, B, H, W, _, _, ref, gc, gd = _setup(oracle, case)
    g, _, _ = ref.grads(gc, gd)
    for k in ("mv_mats", "proj_mats"):
        fd = ref.finite_differences(k, gc, gd)
        assert np.abs(g[k]).max() > 1e-3, k
        assert rel_err(g[k], fd) <= 1e-6, (k, rel_err(g[k], fd))


def _run(r, d, needs_mats=True):
    names = ("verts", "verts_color", "faces_opacity", "verts_depth", "faces_intense") + (("mv_mats", "proj_mats") if needs_mats else ())
    leaves = {k: d[k].clone().requires_grad_(True) for k in names}
    mats = [leaves.get(k, d[k]) for k in ("mv_mats", "proj_mats")]
    color, depth, _ = r(leaves["verts"], d["faces"], leaves["verts_color"], leaves["faces_opacity"], *mats,
                        leaves["verts_depth"], leaves["faces_intense"], d["tets"], d["face_tets"], d["tet_faces"])
    (color.sum() + depth.sum()).backward()
    return leaves


@pytest.mark.parametrize("mode", ["default", "full", "camera", "camera_no_mats"])
def test_module_routes_camera_grads(monkeypatch, mode):
    import dmesh_renderer_amd as dmr
    fake = _FakeC()
    monkeypatch.setattr(dmr._C, "render_tets", fake.render_tets)
    monkeypatch.setattr(dmr._C, "render_tets_backward", fake.render_tets_backward)
    B, H, W = 2, 32, 48
    d = scenes.kuhn_tets(2, B, H, W)
    settings = dmr.TetRenderSettings(H, W, d["bg"], 0)
    r = {"default": lambda: dmr.TetRenderer(settings), "full": lambda: dmr.TetRenderer(settings, full_grads=True)}.get(
        mode, lambda: dmr.TetRenderer(settings, camera_grads=True))()
    leaves = _run(r, d, needs_mats=mode != "camera_no_mats")
    assert len(fake.calls) == 1
    nargs, kw = fake.calls[0]
    assert nargs == 20
    assert th.all(leaves["verts_color"].grad == 2.0) and th.all(leaves["faces_opacity"].grad == 3.0)
    assert leaves["verts_depth"].grad is None
    if mode == "default":  # the reference's call: no new keyword, no new gradient
        assert kw == {"rows": (0, 0)}
        assert leaves["verts"].grad is None and leaves["mv_mats"].grad is None
    elif mode in ("full", "camera_no_mats"):  # camera_grads without a matrix that needs a gradient: the full call
        assert kw == {"rows": (0, 0), "full_grads": True}
        assert th.all(leaves["verts"].grad == 1.0) and th.all(leaves["faces_intense"].grad == 4.0)
        if mode == "full":
            assert leaves["mv_mats"].grad is None and leaves["proj_mats"].grad is None
    else:
        assert kw == {"rows": (0, 0), "camera_grads": True}
        assert th.all(leaves["verts"].grad == 1.0) and th.all(leaves["faces_intense"].grad == 4.0)
        # zero inverse-matrix gradients: only the direct terms, transposed back to the Module's row-major matrices
        assert th.all(leaves["mv_mats"].grad == 5.0) and th.all(leaves["proj_mats"].grad == 6.0)


def test_module_chains_inverse_gradients(monkeypatch):
    """dL/dinv_mv and dL/dinv_proj reach the matrices through -Y^T g Y^T (Y the inverse), added to the direct terms."""
    import dmesh_renderer_amd as dmr
    B, H, W = 1, 32, 32
    d = scenes.kuhn_tets(2, B, H, W)
    g_inv = th.randn(2, B, 4, 4, generator=th.Generator().manual_seed(3), dtype=th.float64).float()
    fake = _FakeC()

    def backward(*args, **kw):
        g = fake.render_tets_backward(*args, **kw)
        return g[:4] + (g_inv[0], g_inv[1]) + g[6:]
    monkeypatch.setattr(dmr._C, "render_tets", fake.render_tets)
    monkeypatch.setattr(dmr._C, "render_tets_backward", backward)
    leaves = _run(dmr.TetRenderer(dmr.TetRenderSettings(H, W, d["bg"], 0), camera_grads=True), d)
    for k, gi, direct in (("mv_mats", g_inv[0], 5.0), ("proj_mats", g_inv[1], 6.0)):
        y = th.inverse(d[k].transpose(1, 2))
        want = (direct - y.transpose(1, 2) @ gi @ y.transpose(1, 2)).transpose(1, 2)
        assert th.allclose(leaves[k].grad, want, rtol=1e-5, atol=1e-5), k


def test_sharded_module_routes_camera_grads():
    """ShardedTetRenderer(camera_grads=True) on one rank through an impl without flat_out support."""
    from dmesh_renderer_amd import TetRenderSettings, sharding
    fake = _FakeC()
    B, H, W = 1, 32, 32
    d = scenes.kuhn_tets(2, B, H, W)
    for cam in (False, True):
        fake.calls.clear()
        sh = sharding.ShardedTetRenderer(TetRenderSettings(H, W, d["bg"], 0), impl=fake, camera_grads=cam)
        leaves = _run(sh, d)
        assert fake.calls[0][1].get("camera_grads", False) == cam
        assert "full_grads" not in fake.calls[0][1]
        assert (leaves["mv_mats"].grad is not None) == cam and (leaves["verts"].grad is not None) == cam
        if cam:
            assert th.all(leaves["mv_mats"].grad == 5.0) and th.all(leaves["proj_mats"].grad == 6.0)


def test_header_declares_flag_and_buffer():
    with open(os.path.join(ROOT, "include", "dmesh_renderer_amd.h")) as f:
        src = f.read()
    assert re.search(r"#define\s+DMR_FLAG_TET_CAMERA_GRADS\s+16\b", src)
    assert re.search(r"\bDMR_BUF_TET_CAMERA_GRADS\s*=\s*7\b", src)
    assert re.search(r"#define\s+DMR_ABI_VERSION\s+4\b", src)


def _gloo_worker(rank, world, port):
    import torch.distributed as dist
    from dmesh_renderer_amd import TetRenderSettings, sharding
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        B, H, W = 1, 64, 32
        d = scenes.kuhn_tets(2, B, H, W)
        fake = _FakeC()
        sh = sharding.ShardedTetRenderer(TetRenderSettings(H, W, d["bg"], 0), impl=fake, camera_grads=True)
        assert sh.world == world and sh.rows != (0, 0)
        leaves = _run(sh, d)
        assert fake.calls[0][1] == {"rows": sh.rows, "camera_grads": True}
        # every rank's gradients summed by the all-reduce
        assert th.all(leaves["mv_mats"].grad == 5.0 * world) and th.all(leaves["proj_mats"].grad == 6.0 * world)
        assert th.all(leaves["verts"].grad == 1.0 * world)
    finally:
        dist.destroy_process_group()


def test_sharded_module_routes_camera_grads_on_gloo():
    """ShardedTetRenderer(camera_grads=True) on two gloo ranks (CPU, stand-in kernels): the keyword reaches every rank's
    backward and the matrix gradients are summed over the ranks."""
    import torch.multiprocessing as mp
    mp.spawn(_gloo_worker, args=(2, free_port()), nprocs=2, join=True)
