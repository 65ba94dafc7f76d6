"""Tet camera gradients on the GPU (DMR_FLAG_TET_CAMERA_GRADS / TetRenderer(camera_grads=True)): dL/dmv_mats and
dL/dproj_mats of both backward kernels against the float64 model of tests/tet_camera_grad_ref.py, on the pixels that
model keeps (the upstream gradients of every other pixel are zeroed on both sides).

The binding returns the gradients of the inverse matrices and the direct ones; they are checked through the chain the
autograd Function applies (direct + _through_inverse).  Bounds: the matrices rel_err <= 1e-3 (rel_err: max-abs error over
max(1, max-abs reference)); the four full gradients within 1e-5 of the full_grads=True call; the re-marching and the
sequence kernel within 1e-5 of each other; the translation identity within 1e-4.  The errors measured on the MI355X are
printed by each case (pytest -s) and recorded in the docstring of test_camera_grads_match_float64_reference.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch as th

from dmesh_renderer_amd import _through_inverse, scenes
from tet_camera_grad_ref import TetCameraGradRef
from util import c_args, rel_err, upstream_grads

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))

MATS_TOL = 1e-3
SAME_TOL = 1e-5
ID_TOL = 1e-4

CASES = {
    # name: (m, B, H, W, opacity, ray_random_seed) -- test_tet_full_grads_gpu.py's cases
    "small": (4, 1, 128, 128, (0.02, 0.3), 0),
    "two_views_ragged": (5, 2, 120, 200, (0.05, 0.5), 0),
    "opaque": (6, 1, 96, 96, (0.6, 1.0), 0),
    "jitter": (5, 2, 112, 144, (0.05, 0.5), 11),
}


def _scene(case, W_extra=0):
    m, B, H, W, op, seed = CASES[case]
    W = W + W_extra
    d = scenes.kuhn_tets(m, B, H, W, seed=0, opacity=op)
    if case == "opaque":
        d["faces_opacity"][::7] = 1.0
    return d, B, H, W, seed


def _reference(oracle, d, B, H, W, seed):
    sc = oracle.scene_from_module_inputs(d, H, W, seed=seed)
    _, _, _, ost = oracle.tet_forward(sc)
    ref = TetCameraGradRef(d, H, W, ost, seed=seed)
    assert ref.kept_fraction >= 0.8, ref.kept_fraction
    gc, gd = upstream_grads(B, H, W)
    m = ref.mask()
    gc, gd = gc * m, gd * m
    g, _, _ = ref.grads(gc, gd)
    return ref, gc, gd, g


def _module_mats(args, g):
    """dL/dmv_mats, dL/dproj_mats of the row-major Module matrices from render_tets_backward(camera_grads=True)'s
    outputs g[4:8] (gradients of the transposed tensors args[5:9]): direct term + chain through the inverse."""
    g_mv = g[6] + _through_inverse(args[7], g[4])
    g_proj = g[7] + _through_inverse(args[8], g[5])
    return g_mv.transpose(1, 2).cpu().numpy(), g_proj.transpose(1, 2).cpu().numpy()


def _identity(d, g):
    """Translating the camera and the mesh together leaves the image fixed: sum of dL/dverts + the translation column of
    dL/dinv_mv - mv[:, 0:3]^T dL/dmv's translation column = 0 (normalised by the sum of |dL/dverts|)."""
    g = [x.cpu().numpy().astype(np.float64) for x in g]
    mv = d["mv_mats"].numpy().astype(np.float64)            # row-major
    col = g[4][:, 3, :3] - np.einsum("bi,bij->bj", g[6][:, 3, :], mv[:, :, :3])  # [b, 3, i] of a returned tensor = [i][3]
    return float(np.abs(col.sum(0) + g[0].sum(0)).max()) / max(float(np.abs(g[0]).sum()), 1e-30)


def _seq_state(_C, args, bufs, H, W):
    longest, cap = _C.export("tet_seq", args, True, 0, bufs, H, W, th.int32).cpu().numpy().view(np.uint32)[:2]
    return int(longest), int(cap)


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
    d, B, H, W, seed = _scene(case, W_extra=16 * (13 + list(CASES).index(case)))  # a view configuration of its own
    ref, gc, gd, rg = _reference(oracle, d, B, H, W, seed)
    args = c_args(d, hip_device, tet=True)
    gcd, gdd = gc.to(hip_device), gd.to(hip_device)
    cams = []
    for call in range(2):
        out = _C.render_tets(*args, H, W, seed)
        gk = _C.render_tets_backward(*args, gcd, gdd, *out[3:7], camera_grads=True)
        gf = _C.render_tets_backward(*args, gcd, gdd, *out[3:7], full_grads=True)
        th.cuda.synchronize()
        longest, cap = _seq_state(_C, args, out[3:7], H, W)
        assert (cap == 0) if call == 0 else (0 < longest <= cap), (call, longest, cap)
        assert len(gk) == 8 and all(x.shape == (B, 4, 4) for x in gk[4:])
        g_mv, g_proj = _module_mats(args, gk)
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
    d, B, H, W, seed = _scene("two_views_ragged")
    ref, gc, gd, rg = _reference(oracle, d, B, H, W, seed)
    t = {k: v.to(hip_device) for k, v in d.items()}
    names = ("verts", "verts_color", "faces_opacity", "mv_mats", "proj_mats", "verts_depth", "faces_intense")
    leaves = {k: t[k].clone().requires_grad_(True) for k in names}
    r = dmr.TetRenderer(dmr.TetRenderSettings(H, W, t["bg"], seed), camera_grads=True)
    color, depth, _ = r(leaves["verts"], t["faces"], leaves["verts_color"], leaves["faces_opacity"], leaves["mv_mats"],
                        leaves["proj_mats"], leaves["verts_depth"], leaves["faces_intense"], t["tets"], t["face_tets"], t["tet_faces"])
    th.autograd.backward([color, depth], [gc.to(hip_device), gd.to(hip_device)])
    assert leaves["verts_depth"].grad is None
    for k in ("mv_mats", "proj_mats"):
        assert rel_err(leaves[k].grad.cpu().numpy(), rg[k]) <= MATS_TOL, k
    assert rel_err(leaves["verts"].grad.cpu().numpy(), rg["verts"]) <= 1e-3
    assert rel_err(leaves["verts_color"].grad.cpu().numpy(), rg["verts_color"]) <= 1e-4


def test_camera_grads_step_replays_as_graph(hip_device):
    """One forward + camera-gradient backward captured with torch.cuda.graph matches the eager call."""
    from dmesh_renderer_amd import _C
    d, B, H, W, seed = _scene("two_views_ragged", W_extra=16 * 17)
    args = c_args(d, hip_device, tet=True)
    gc, gd = upstream_grads(B, H, W)
    gcd, gdd = gc.to(hip_device), gd.to(hip_device)

    def step():
        out = _C.render_tets(*args, H, W, seed)
        return _C.render_tets_backward(*args, gcd, gdd, *out[3:7], camera_grads=True)

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
from dmesh_renderer_amd import _C, _through_inverse, scenes
from dmesh_renderer_amd.scenes import c_args, rel_err
from oracle import oracle as O
from tet_camera_grad_ref import TetCameraGradRef
from util import upstream_grads
O.build()
dev = th.device("cuda:0")
B, H, W = 2, 120, 232
d = scenes.kuhn_tets(5, B, H, W, seed=0, opacity=(0.05, 0.5))
sc = O.scene_from_module_inputs(d, H, W)
_, _, _, ost = O.tet_forward(sc)
ref = TetCameraGradRef(d, H, W, ost)
gc, gd = upstream_grads(B, H, W)
m = ref.mask(); gc, gd = gc * m, gd * m
rg, _, _ = ref.grads(gc, gd)
args = c_args(d, dev, tet=True)
for call in range(2):  # re-marching kernel, then the sequence kernel
    out = _C.render_tets(*args, H, W, 0)
    g = _C.render_tets_backward(*args, gc.to(dev), gd.to(dev), *out[3:7], camera_grads=True)
    g_mv = (g[6] + _through_inverse(args[7], g[4])).transpose(1, 2).cpu().numpy()
    g_proj = (g[7] + _through_inverse(args[8], g[5])).transpose(1, 2).cpu().numpy()
    assert rel_err(g_mv, rg["mv_mats"]) <= %r, (call, "mv")
    assert rel_err(g_proj, rg["proj_mats"]) <= %r, (call, "proj")
    assert rel_err(g[0].cpu().numpy(), rg["verts"]) <= 1e-3, (call, "verts")
    assert rel_err(g[1].cpu().numpy(), rg["verts_color"]) <= 1e-4, (call, "verts_color")
print("camera fallback ok")
"""


def test_camera_grads_direct_atomic_fallback(hip_device):
    """The camera variant with the direct-atomic fallback: the ablation build with DMR_ABLATE=2048 refuses odd faces a
    table slot (as tests/test_fallback_gpu.py does for the default gradients)."""
    from dmesh_renderer_amd import build
    lib = build.build(ablation=True)
    env = dict(os.environ, DMR_ABLATE="2048", DMR_LIBRARY=lib)
    r = subprocess.run([sys.executable, "-c", FALLBACK_CHILD % (ROOT, HERE, MATS_TOL, MATS_TOL)], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and "camera fallback ok" in r.stdout, r.stdout + r.stderr


def test_two_ranks_camera_grads_match_single_rank(hip_device):
    """ShardedTetRenderer(camera_grads=True) on two ranks (gloo, one GPU) against TetRenderer(camera_grads=True) alone."""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29543", os.path.join(HERE, "sharded_camera_grads_child.py")]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=400)
    assert r.returncode == 0 and "sharded camera grads ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
