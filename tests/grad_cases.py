"""The cases, the reference set-up and the bounds of the opt-in gradient tests (tri exact / camera, tet full, tet camera),
once per renderer: tests/test_{tri_exact,tet_full,tet_camera}_grads_{gpu,cpu}.py, tests/test_alpha_gpu.py and
tests/fallback_child.py import from here.  rel_err: max-abs error over max(1, max-abs reference)."""
import numpy as np
import torch as th

from dmesh_renderer_amd import _through_inverse, scenes
from tet_camera_grad_ref import TetCameraGradRef
from tet_grad_ref import TetGradRef
from tri_grad_ref import TriGradRef
from util import upstream_grads, with_bg

TRI_VERTS_TOL = 1e-4   # dL_dverts against the float64 model
TET_VERTS_TOL = 1e-3
FINT_TOL = 1e-4        # tet dL_dfaces_intense
MATS_TOL = CAM_TOL = 1e-3  # dL_dmv_mats, dL_dproj_mats (tet / tri name)
SAME_TOL = 1e-5        # two paths that compute the same sums
ID_TOL = 1e-4          # the translation identity

TET_CASES = {
    # name: (m, B, H, W, opacity, ray_random_seed) -- test_tet_parity_gpu.py's cases plus seeded jitter
    "small": (4, 1, 128, 128, (0.02, 0.3), 0),
    "two_views_ragged": (5, 2, 120, 200, (0.05, 0.5), 0),
    "opaque": (6, 1, 96, 96, (0.6, 1.0), 0),
    "jitter": (5, 2, 112, 144, (0.05, 0.5), 11),
}

TRI_CASES = {
    # name: (L, n, B, H, W, rows)
    "one_view": (3, 9, 1, 96, 128, (0, 0)),
    "two_views_ragged": (3, 8, 2, 88, 152, (0, 0)),
    "band": (3, 9, 2, 96, 128, (1, 4)),
}


def scene(case, W_extra=0, cases=TET_CASES, bg=None):
    """The tet scene of a case; W_extra widens the frame, which gives a test a view configuration of its own; bg: its
    background (default: the scene's own, zero)."""
    m, B, H, W, op, seed = cases[case]
    W = W + W_extra
    d = scenes.kuhn_tets(m, B, H, W, seed=0, opacity=op)
    if case == "opaque":
        d["faces_opacity"][::7] = 1.0
    if bg is not None:
        d = with_bg(d, bg)
    return d, B, H, W, seed


def reference(oracle, d, B, H, W, seed, camera=False):
    """The float64 model of a tet scene, the upstream gradients masked to the pixels it keeps, and its gradients."""
    sc = oracle.scene_from_module_inputs(d, H, W, seed=seed)
    _, _, _, ost = oracle.tet_forward(sc)
    ref = TetCameraGradRef(d, H, W, ost, seed=seed) if camera else TetGradRef(d, H, W, ost)
    assert ref.kept_fraction >= 0.8, ref.kept_fraction
    gc, gd = upstream_grads(B, H, W)
    m = ref.mask()
    gc, gd = gc * m, gd * m
    g, _, _ = ref.grads(gc, gd)
    return ref, gc, gd, g


def seq_state(_C, args, bufs, H, W):
    """(longest march sequence, capacity) of the tet forward state: capacity 0 on the first call of a view configuration."""
    longest, cap = _C.export("tet_seq", args, True, 0, bufs, H, W, th.int32).cpu().numpy().view(np.uint32)[:2]
    return int(longest), int(cap)


def module_mats(args, g):
    """dL/dmv_mats, dL/dproj_mats of the row-major Module matrices from render_tets_backward(camera_grads=True)'s
    outputs g[4:8] (gradients of the transposed tensors args[5:9]): direct term + chain through the inverse."""
    g_mv = g[6] + _through_inverse(args[7], g[4])
    g_proj = g[7] + _through_inverse(args[8], g[5])
    return g_mv.transpose(1, 2).cpu().numpy(), g_proj.transpose(1, 2).cpu().numpy()


def setup(oracle, case, bg=None, W_extra=0):
    """The tri scene of a case (bg: its background, default the scene's own, zero; W_extra widens the frame, as for scene),
    the upstream gradients masked to the pixels the float64 model keeps, its gradients."""
    L, n, B, H, W, rows = TRI_CASES[case]
    W = W + W_extra
    d = scenes.layered_sheets(L, n, B, H, W, seed=7, opacity=(0.1, 0.5))
    if bg is not None:
        d = with_bg(d, bg)
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
