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
import numpy as np
import pytest
import torch as th

from dmesh_renderer_amd import scenes
from grad_cases import CAM_TOL, ID_TOL, SAME_TOL, TRI_CASES as CASES, TRI_VERTS_TOL as VERTS_TOL, setup
from harness import capture_replay, module_step, replay, run_ablation_child, run_ranks
from util import c_args, rel_err, upstream_grads

pytestmark = pytest.mark.gpu


def _identity(g_verts, g_inv_mv):
    """Translation column of dL/dinv_mv (element [b, 3, 0:3] of the returned tensor) = -sum of the vertex gradients."""
    scale = float(np.abs(g_verts).sum())
    return float(np.abs(g_inv_mv[:, 3, :3].sum(0) + g_verts.sum(0)).max()) / max(scale, 1e-30)


@pytest.mark.parametrize("case", list(CASES))
def test_exact_and_camera_grads_match_float64_model(oracle, hip_device, case):
    """The _C call with exact_grads and with camera_grads against the model and against the default call."""
    from dmesh_renderer_amd import _C
    d, B, H, W, rows, gc, gd, rg = setup(oracle, case)
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
    d, B, H, W, rows, gc, gd, rg = setup(oracle, case)
    t = {k: v.to(hip_device) for k, v in d.items()}
    r = dmr.TriRenderer(dmr.TriRenderSettings(H, W, t["bg"]), camera_grads=True)
    _, g = module_step(r, t, ("verts", "verts_color", "faces_opacity", "mv_mats", "proj_mats", "verts_depth", "faces_intense"),
                       [gc.to(hip_device), gd.to(hip_device)])
    em = rel_err(g["mv_mats"].cpu().numpy(), rg["mv_mats"])
    ep = rel_err(g["proj_mats"].cpu().numpy(), rg["proj_mats"])
    ev = rel_err(g["verts"].cpu().numpy(), rg["verts"])
    print(f"\n{case}: dL_dmv_mats {em:.2e}  dL_dproj_mats {ep:.2e}  dL_dverts {ev:.2e}  "
          f"(|dL_dmv| {np.abs(rg['mv_mats']).max():.3g}, |dL_dproj| {np.abs(rg['proj_mats']).max():.3g})")
    assert em <= CAM_TOL and ep <= CAM_TOL, (em, ep)
    assert ev <= VERTS_TOL
    for k in ("verts_color", "faces_opacity", "verts_depth", "faces_intense"):
        assert rel_err(g[k].cpu().numpy(), rg[k]) <= 1e-4, k


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

    graph, captured, eager = capture_replay(step)
    replay(graph)
    for a, b_ in zip(captured, eager):
        assert rel_err(a.cpu().numpy(), b_.cpu().numpy()) <= SAME_TOL


def test_exact_grads_direct_atomic_fallback(hip_device):
    """The exact rows through the direct atomics: the ablation build (harness.run_ablation_child) refuses odd vertex rows a table
    slot (as tests/test_fallback_gpu.py does for the default gradients)."""
    run_ablation_child("tri_exact", "exact fallback ok")


def test_two_ranks_camera_grads_match_single_rank(hip_device):
    """ShardedTriRenderer(camera_grads=True), both partitions, two ranks (gloo, one GPU) against TriRenderer alone."""
    run_ranks("exact_grads", "sharded exact grads ok")
