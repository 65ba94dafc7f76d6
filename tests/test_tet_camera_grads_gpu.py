"""Tet camera gradients on the GPU (DMR_FLAG_TET_CAMERA_GRADS / TetRenderer(camera_grads=True)): dL/dmv_mats and
dL/dproj_mats of both backward kernels against the float64 model of tests/tet_camera_grad_ref.py, on the pixels that
model keeps (the upstream gradients of every other pixel are zeroed on both sides).

The binding returns the gradients of the inverse matrices and the direct ones; they are checked through the chain the
autograd Function applies (direct + _through_inverse).  Bounds: the matrices rel_err <= 1e-3 (rel_err: max-abs error over
max(1, max-abs reference)); the four full gradients within 1e-5 of the full_grads=True call; the re-marching and the
sequence kernel within 1e-5 of each other; the translation identity within 1e-4.  The errors measured on the MI355X are
printed by each case (pytest -s) and recorded in the docstring of test_camera_grads_match_float64_reference.
"""
import numpy as np
import pytest
import torch as th

from grad_cases import ID_TOL, MATS_TOL, SAME_TOL, TET_CASES as CASES, module_mats, reference, scene, seq_state
from harness import capture_replay, module_step, replay, run_ablation_child, run_ranks
from util import c_args, rel_err, upstream_grads

pytestmark = pytest.mark.gpu


def _identity(d, g):
    """Translating the camera and the mesh together leaves the image fixed: sum of dL/dverts + the translation column of
    dL/dinv_mv - mv[:, 0:3]^T dL/dmv's translation column = 0 (normalised by the sum of |dL/dverts|)."""
    g = [x.cpu().numpy().astype(np.float64) for x in g]
    mv = d["mv_mats"].numpy().astype(np.float64)            # row-major
    col = g[4][:, 3, :3] - np.einsum("bi,bij->bj", g[6][:, 3, :], mv[:, :, :3])  # [b, 3, i] of a returned tensor = [i][3]
    return float(np.abs(col.sum(0) + g[0].sum(0)).max()) / max(float(np.abs(g[0]).sum()), 1e-30)


@pytest.mark.parametrize("case", list(CASES))
def test_camera_grads_match_float64_reference(oracle, hip_device, case):
    """First call of a view configuration (the re-marching k_tet_backward) and second call (k_tet_backward_seq), each
    with camera gradients and with the full ones.
    Measured on the MI355X (rel_err dL_dmv / dL_dproj, translation identity; call 0 and call 1; kept pixels):
      small             8.1e-7 / 4.5e-7, 1.2e-8;  9.0e-7 / 2.2e-7, 1.3e-8  (97 %)
      two_views_ragged  8.3e-7 / 1.0e-6, 2.5e-8;  1.1e-6 / 7.1e-7, 2.5e-8  (97 %)
      opaque            2.7e-7 / 5.3e-7, 9.2e-9;  3.7e-7 / 1.5e-7, 1.4e-8  (92 %)
      jitter            1.3e-6 / 2.2e-6, 1.2e-8;  1.1e-6 / 1.9e-6, 5.9e-9  (96 %)"""
    from dmesh_renderer_amd import _C
    d, B, H, W, seed = scene(case, W_extra=16 * (13 + list(CASES).index(case)))  # a view configuration of its own
    ref, gc, gd, rg = reference(oracle, d, B, H, W, seed, camera=True)
    args = c_args(d, hip_device, tet=True)
    gcd, gdd = gc.to(hip_device), gd.to(hip_device)
    cams = []
    for call in range(2):
        out = _C.render_tets(*args, H, W, seed)
        gk = _C.render_tets_backward(*args, gcd, gdd, *out[3:7], camera_grads=True)
        gf = _C.render_tets_backward(*args, gcd, gdd, *out[3:7], full_grads=True)
        th.cuda.synchronize()
        longest, cap = seq_state(_C, args, out[3:7], H, W)
        assert (cap == 0) if call == 0 else (0 < longest <= cap), (call, longest, cap)
        assert len(gk) == 8 and all(x.shape == (B, 4, 4) for x in gk[4:])
        g_mv, g_proj = module_mats(args, gk)
        em, ep = rel_err(g_mv, rg["mv_mats"]), rel_err(g_proj, rg["proj_mats"])
        ei = _identity(d, gk)
        print(f"\n{case} call {call}: dL_dmv {em:.2e}  dL_dproj {ep:.2e}  identity {ei:.2e}  kept {ref.kept_fraction:.3f}")
        assert em <= MATS_TOL and ep <= MATS_TOL, (call, em, ep)
        assert ei <= ID_TOL, (call, ei)
        for a, b_ in zip(gk[:4], gf):
            assert rel_err(a.cpu().numpy(), b_.cpu().numpy()) <= SAME_TOL
        cams.append([x.cpu().numpy() for x in gk])
    for a, b_ in zip(cams[0], cams[1]):  # re-march vs sequence kernel
        assert rel_err(a, b_) <= SAME_TOL


def test_module_camera_grads_two_views(oracle, hip_device):
    """TetRenderer(camera_grads=True) through autograd, B = 2."""
    import dmesh_renderer_amd as dmr
    d, B, H, W, seed = scene("two_views_ragged")
    ref, gc, gd, rg = reference(oracle, d, B, H, W, seed, camera=True)
    t = {k: v.to(hip_device) for k, v in d.items()}
    r = dmr.TetRenderer(dmr.TetRenderSettings(H, W, t["bg"], seed), camera_grads=True)
    _, g = module_step(r, t, ("verts", "verts_color", "faces_opacity", "mv_mats", "proj_mats", "verts_depth", "faces_intense"),
                       [gc.to(hip_device), gd.to(hip_device)])
    assert g["verts_depth"] is None
    for k in ("mv_mats", "proj_mats"):
        assert rel_err(g[k].cpu().numpy(), rg[k]) <= MATS_TOL, k
    assert rel_err(g["verts"].cpu().numpy(), rg["verts"]) <= 1e-3
    assert rel_err(g["verts_color"].cpu().numpy(), rg["verts_color"]) <= 1e-4


def test_camera_grads_step_replays_as_graph(hip_device):
    """One forward + camera-gradient backward captured with torch.cuda.graph matches the eager call."""
    from dmesh_renderer_amd import _C
    d, B, H, W, seed = scene("two_views_ragged", W_extra=16 * 17)
    args = c_args(d, hip_device, tet=True)
    gc, gd = upstream_grads(B, H, W)
    gcd, gdd = gc.to(hip_device), gd.to(hip_device)

    def step():
        out = _C.render_tets(*args, H, W, seed)
        return _C.render_tets_backward(*args, gcd, gdd, *out[3:7], camera_grads=True)

    graph, captured, eager = capture_replay(step)
    replay(graph)
    for a, b_ in zip(captured, eager):
        assert rel_err(a.cpu().numpy(), b_.cpu().numpy()) <= SAME_TOL


def test_camera_grads_direct_atomic_fallback(hip_device):
    """The camera variant with the direct-atomic fallback: the ablation build (harness.run_ablation_child) refuses odd faces a
    table slot (as tests/test_fallback_gpu.py does for the default gradients)."""
    run_ablation_child("tet_camera", "camera fallback ok")


def test_two_ranks_camera_grads_match_single_rank(hip_device):
    """ShardedTetRenderer(camera_grads=True) on two ranks (gloo, one GPU) against TetRenderer(camera_grads=True) alone."""
    run_ranks("camera_grads_tet", "sharded camera grads ok")
