"""Exact vertex gradients and camera gradients of the tri renderer on the GPU (DMR_FLAG_TRI_EXACT_GRADS /
DMR_FLAG_TRI_CAMERA_GRADS, TriRenderer(exact_grads=True, camera_grads=True)) against the float64 model of
tests/tri_grad_ref.py, on the pixels that model keeps (the upstream gradients of every other pixel are zeroed on both
sides).

Bounds: dL_dverts rel_err <= 1e-4; dL_dmv_mats, dL_dproj_mats <= 1e-3; verts_color / faces_opacity / verts_depth /
faces_intense within 1e-5 of the default path's (rel_err: max-abs error over max(1, max-abs reference)).  The errors
measured on the MI355X are printed by each case (pytest -s): dL_dverts 1.6e-6 (one_view), 1.2e-6 (two_views_ragged),
7.3e-7 (band), where the reference's gradient is 0.74-1.18 off; dL_dmv_mats 8.2e-7, dL_dproj_mats 4.8e-7; translation
identity <= 2.1e-8.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch as th

from dmesh_renderer_amd import scenes
from tri_grad_ref import TriGradRef
from util import c_args, rel_err, upstream_grads

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))

VERTS_TOL = 1e-4
CAM_TOL = 1e-3
SAME_TOL = 1e-5
ID_TOL = 1e-4

CASES = {
    # name: (L, n, B, H, W, rows)
    "one_view": (3, 9, 1, 96, 128, (0, 0)),
    "two_views_ragged": (3, 8, 2, 88, 152, (0, 0)),
    "band": (3, 9, 2, 96, 128, (1, 4)),
}


def _setup(oracle, case):
    L, n, B, H, W, rows = CASES[case]
    d = scenes.layered_sheets(L, n, B, H, W, seed=7, opacity=(0.1, 0.5))
    sc = oracle.scene_from_module_inputs(d, H, W)
    _, _, ost = oracle.tri_forward(sc)
    ref = TriGradRef(d, H, W, ost)
    assert ref.kept_fraction >= 0.8, ref.kept_fraction
    gc, gd = upstream_grads(B, H, W)
    m = ref.mask()
    if rows != (0, 0):  # a band: the pixels outside it are not rendered, their upstream gradients do not matter
        m = m.clone()
        m[:, :, :16 * rows[0]] = 0
        m[:, :, 16 * rows[1]:] = 0
    gc, gd = gc * m, gd * m
    rg, _, _ = ref.grads(gc, gd)
    return d, B, H, W, rows, gc, gd, rg


def _identity(g_verts, g_inv_mv):
    """Translation column of dL/dinv_mv (element [b, 3, 0:3] of the returned tensor) = -sum of the vertex gradients."""
    scale = float(np.abs(g_verts).sum())
    return float(np.abs(g_inv_mv[:, 3, :3].sum(0) + g_verts.sum(0)).max()) / max(scale, 1e-30)


@pytest.mark.parametrize("case", list(CASES))
def test_exact_and_camera_grads_match_float64_model(oracle, hip_device, case):
    """The _C call with exact_grads and with camera_grads against the model and against the default call."""
    from dmesh_renderer_amd import _C
    d, B, H, W, rows, gc, gd, rg = _setup(oracle, case)
    args = c_args(d, hip_device)
    gcd, gdd = gc.to(hip_device), gd.to(hip_device)
    for call in range(2):  # the first backward of a view configuration (scanned record regions), then a later one
        out = _C.render_tris(*args, H, W, rows=rows)
        g0 = [x.cpu().numpy() for x in _C.render_tris_backward(*args, gcd, gdd, out[0], *out[3:7], rows=rows)]
        ge = [x.cpu().numpy() for x in _C.render_tris_backward(*args, gcd, gdd, out[0], *out[3:7], rows=rows, exact_grads=True)]
        gk = [x.cpu().numpy() for x in _C.render_tris_backward(*args, gcd, gdd, out[0], *out[3:7], rows=rows, camera_grads=True)]
        assert len(ge) == 5 and len(gk) == 7 and gk[5].shape == (B, 4, 4) and gk[6].shape == (B, 4, 4)
        ev, ek = rel_err(ge[0], rg["verts"]), rel_err(gk[0], rg["verts"])
        print(f"\n{case} call {call}: dL_dverts exact {ev:.2e} camera {ek:.2e}  (reference's {rel_err(g0[0], rg['verts']):.2e})")
        assert ev <= VERTS_TOL and ek <= VERTS_TOL, (ev, ek)
        for i in range(1, 5):
            assert rel_err(ge[i], g0[i]) <= SAME_TOL and rel_err(gk[i], g0[i]) <= SAME_TOL, i
        # the ray origin and the three vertices enter (u, v) only as differences
        if B == 1:
            e = _identity(gk[0], gk[5])
            print(f"{case}: translation identity {e:.2e}")
            assert e <= ID_TOL, e


@pytest.mark.parametrize("case", ["one_view", "two_views_ragged"])
def test_module_camera_grads_match_float64_model(oracle, hip_device, case):
    """TriRenderer(camera_grads=True) through autograd: dL/dmv_mats, dL/dproj_mats of the row-major Module inputs."""
    import dmesh_renderer_amd as dmr
    d, B, H, W, rows, gc, gd, rg = _setup(oracle, case)
    t = {k: v.to(hip_device) for k, v in d.items()}
    names = ("verts", "verts_color", "faces_opacity", "mv_mats", "proj_mats", "verts_depth", "faces_intense")
    leaves = {k: t[k].clone().requires_grad_(True) for k in names}
    r = dmr.TriRenderer(dmr.TriRenderSettings(H, W, t["bg"]), camera_grads=True)
    color, depth = r(*(leaves[k] if k in leaves else t[k] for k in ("verts", "faces", "verts_color", "faces_opacity", "mv_mats",
                                                                     "proj_mats", "verts_depth", "faces_intense")))
    th.autograd.backward([color, depth], [gc.to(hip_device), gd.to(hip_device)])
    em = rel_err(leaves["mv_mats"].grad.cpu().numpy(), rg["mv_mats"])
    ep = rel_err(leaves["proj_mats"].grad.cpu().numpy(), rg["proj_mats"])
    ev = rel_err(leaves["verts"].grad.cpu().numpy(), rg["verts"])
    print(f"\n{case}: dL_dmv_mats {em:.2e}  dL_dproj_mats {ep:.2e}  dL_dverts {ev:.2e}  "
          f"(|dL_dmv| {np.abs(rg['mv_mats']).max():.3g}, |dL_dproj| {np.abs(rg['proj_mats']).max():.3g})")
    assert em <= CAM_TOL and ep <= CAM_TOL, (em, ep)
    assert ev <= VERTS_TOL
    for k in ("verts_color", "faces_opacity", "verts_depth", "faces_intense"):
        assert rel_err(leaves[k].grad.cpu().numpy(), rg[k]) <= 1e-4, k


def test_camera_grads_scanned_path(hip_device):
    """A frame of more than 8 192 tiles (the record regions come from k_scan_hits every call): the four default gradients
    are unchanged and the translation identity holds."""
    from dmesh_renderer_amd import _C
    L, n, B, H, W = 3, 40, 1, 1040, 2048
    assert ((H + 15) // 16) * ((W + 15) // 16) * B > 8192
    d = scenes.layered_sheets(L, n, B, H, W, seed=5, opacity=(0.1, 0.5))
    d["verts"] = d["verts"] * th.tensor([4.0, 4.0, 1.0])
    args = c_args(d, hip_device)
    gc, gd = upstream_grads(B, H, W)
    gcd, gdd = gc.to(hip_device), gd.to(hip_device)
    for call in range(2):
        out = _C.render_tris(*args, H, W)
        g0 = [x.cpu().numpy() for x in _C.render_tris_backward(*args, gcd, gdd, out[0], *out[3:7])]
        gk = [x.cpu().numpy() for x in _C.render_tris_backward(*args, gcd, gdd, out[0], *out[3:7], camera_grads=True)]
        ge = [x.cpu().numpy() for x in _C.render_tris_backward(*args, gcd, gdd, out[0], *out[3:7], exact_grads=True)]
        for i in range(1, 5):
            assert rel_err(gk[i], g0[i]) <= SAME_TOL, i
        assert rel_err(gk[0], ge[0]) <= SAME_TOL
        e = _identity(gk[0], gk[5])
        print(f"\nscanned call {call}: translation identity {e:.2e}")
        assert e <= ID_TOL, e


def test_camera_grads_step_replays_as_graph(hip_device):
    """One forward + camera-gradient backward captured with torch.cuda.graph matches the eager call."""
    from dmesh_renderer_amd import _C
    L, n, B, H, W, _ = CASES["two_views_ragged"]
    d = scenes.layered_sheets(L, n, B, H, W + 16 * 9, seed=2)
    W = W + 16 * 9
    args = c_args(d, hip_device)
    gc, gd = upstream_grads(B, H, W)
    gcd, gdd = gc.to(hip_device), gd.to(hip_device)

    def step():
        out = _C.render_tris(*args, H, W)
        return _C.render_tris_backward(*args, gcd, gdd, out[0], *out[3:7], camera_grads=True)

    s = th.cuda.Stream()
    s.wait_stream(th.cuda.current_stream())
    with th.cuda.stream(s):
        for _ in range(2):  # the size estimates the capture needs
            eager = [x.clone() for x in step()]
    th.cuda.current_stream().wait_stream(s)
    th.cuda.synchronize()
    _C.overflowed()
    g = th.cuda.CUDAGraph()
    with th.cuda.graph(g):
        captured = step()
    g.replay()
    th.cuda.synchronize()
    assert not _C.overflowed()
    for a, b_ in zip(captured, eager):
        assert rel_err(a.cpu().numpy(), b_.cpu().numpy()) <= SAME_TOL


FALLBACK_CHILD = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np, torch as th
from dmesh_renderer_amd import _C, scenes
from dmesh_renderer_amd.scenes import c_args, rel_err
from oracle import oracle as O
from tri_grad_ref import TriGradRef
from util import upstream_grads
O.build()
dev = th.device("cuda:0")
B, H, W = 1, 96, 128
d = scenes.layered_sheets(3, 9, B, H, W, seed=7, opacity=(0.1, 0.5))
sc = O.scene_from_module_inputs(d, H, W)
_, _, ost = O.tri_forward(sc)
ref = TriGradRef(d, H, W, ost)
gc, gd = upstream_grads(B, H, W)
m = ref.mask(); gc, gd = gc * m, gd * m
rg, _, _ = ref.grads(gc, gd)
og = O.tri_backward(sc, ost, gc.numpy(), gd.numpy())
args = c_args(d, dev)
for call in range(2):
    out = _C.render_tris(*args, H, W)
    for kw in ({"exact_grads": True}, {"camera_grads": True}):
        g = [x.cpu().numpy() for x in _C.render_tris_backward(*args, gc.to(dev), gd.to(dev), out[0], *out[3:7], **kw)]
        assert rel_err(g[0], rg["verts"]) <= %r, (call, kw, rel_err(g[0], rg["verts"]))
        for i, k in enumerate(("verts_color", "faces_opacity", "verts_depth", "faces_intense")):
            assert rel_err(g[1 + i], og[k]) <= 1e-4, (call, kw, k)
    assert np.abs(g[5][:, 3, :3].sum(0) + g[0].sum(0)).max() <= 1e-4 * float(np.abs(g[0]).sum()), call
print("exact fallback ok")
"""


def test_exact_grads_direct_atomic_fallback(hip_device):
    """The exact rows through the direct atomics: the ablation build with DMR_ABLATE=2048 refuses odd vertex rows a table
    slot (as tests/test_fallback_gpu.py does for the default gradients)."""
    from dmesh_renderer_amd import build
    lib = build.build(ablation=True)
    env = dict(os.environ, DMR_ABLATE="2048", DMR_LIBRARY=lib)
    r = subprocess.run([sys.executable, "-c", FALLBACK_CHILD % (ROOT, HERE, VERTS_TOL)], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and "exact fallback ok" in r.stdout, r.stdout + r.stderr


def test_two_ranks_camera_grads_match_single_rank(hip_device):
    """ShardedTriRenderer(camera_grads=True), both partitions, two ranks (gloo, one GPU) against TriRenderer alone."""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29541", os.path.join(HERE, "sharded_exact_grads_child.py")]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=400)
    assert r.returncode == 0 and "sharded exact grads ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
