"""Full tet gradients on the GPU (DMR_FLAG_TET_FULL_GRADS / TetRenderer(full_grads=True)): dL/dverts and
dL/dfaces_intense of both backward kernels against the float64 brute-force reference of tests/tet_grad_ref.py, on the
pixels that reference keeps (the upstream gradients of every other pixel are zeroed on both sides).

Bounds: dL_dverts rel_err <= 1e-3, dL_dfintense <= 1e-4 (rel_err: max-abs error over max(1, max-abs reference)); the
full path's verts_color / faces_opacity within 1e-5 of the default path's; the re-marching and the sequence kernel
within 1e-5 of each other.  The errors measured on the MI355X are printed by each case (pytest -s) and recorded in
the docstring of test_full_grads_match_float64_reference.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch as th

from dmesh_renderer_amd import scenes
from tet_grad_ref import TetGradRef
from util import c_args, rel_err, upstream_grads

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))

VERTS_TOL = 1e-3
FINT_TOL = 1e-4
SAME_TOL = 1e-5

CASES = {
    # name: (m, B, H, W, opacity, ray_random_seed) -- test_tet_parity_gpu.py's cases plus seeded jitter
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
    ref = TetGradRef(d, H, W, ost)
    assert ref.kept_fraction >= 0.8, ref.kept_fraction
    gc, gd = upstream_grads(B, H, W)
    m = ref.mask()
    gc, gd = gc * m, gd * m
    g, _, _ = ref.grads(gc, gd)
    return ref, gc, gd, g


def _seq_state(_C, args, bufs, H, W):
    longest, cap = _C.export("tet_seq", args, True, 0, bufs, H, W, th.int32).cpu().numpy().view(np.uint32)[:2]
    return int(longest), int(cap)


@pytest.mark.parametrize("case", list(CASES))
def test_full_grads_match_float64_reference(oracle, hip_device, case):
    """First call of a view configuration (no march sequence yet: the re-marching k_tet_backward) and second call
    (k_tet_backward_seq on the forward's sequence), each with full gradients and with the default ones.
    Measured on the MI355X (rel_err dL_dverts / dL_dfintense, call 0 and call 1; kept pixels):
      small             5.8e-6 / 2.0e-7, 4.6e-6 / 2.1e-7  (97 %)
      two_views_ragged  4.8e-6 / 3.7e-7, 4.9e-6 / 3.8e-7  (97 %)
      opaque            1.7e-6 / 5.3e-7, 1.7e-6 / 5.3e-7  (92 %)
      jitter            1.2e-5 / 1.9e-7, 9.7e-6 / 2.4e-7  (96 %)
    No criterion on grazing hits (small |den|) was needed.  tet_grad_ref already drops rays that pass within EDGE_EPS of
    a face edge, because the reference's reverse march stops early along them."""
    from dmesh_renderer_amd import _C
    d, B, H, W, seed = _scene(case, W_extra=16 * (6 + list(CASES).index(case)))  # a view configuration of its own
    ref, gc, gd, rg = _reference(oracle, d, B, H, W, seed)
    args = c_args(d, hip_device, tet=True)
    gcd, gdd = gc.to(hip_device), gd.to(hip_device)
    fulls = []
    for call in range(2):
        out = _C.render_tets(*args, H, W, seed)
        gf = _C.render_tets_backward(*args, gcd, gdd, *out[3:7], full_grads=True)
        g0 = _C.render_tets_backward(*args, gcd, gdd, *out[3:7])
        th.cuda.synchronize()
        longest, cap = _seq_state(_C, args, out[3:7], H, W)
        assert (cap == 0) if call == 0 else (0 < longest <= cap), (call, longest, cap)
        gf = [x.cpu().numpy() for x in gf]
        assert gf[0].shape == (d["verts"].shape[0], 3) and gf[3].shape == (B, d["faces"].shape[0])
        ev, ei = rel_err(gf[0], rg["verts"]), rel_err(gf[3], rg["faces_intense"])
        print(f"\n{case} call {call}: dL_dverts {ev:.2e}  dL_dfintense {ei:.2e}  kept {ref.kept_fraction:.3f}")
        assert ev <= VERTS_TOL, (call, ev)
        assert ei <= FINT_TOL, (call, ei)
        for a, b_ in zip(gf[1:3], g0):
            assert rel_err(a, b_.cpu().numpy()) <= SAME_TOL
        fulls.append(gf)
    for a, b_ in zip(fulls[0], fulls[1]):  # re-march vs sequence kernel
        assert rel_err(a, b_) <= SAME_TOL


def test_module_full_grads_two_views(oracle, hip_device):
    """TetRenderer(full_grads=True) through autograd, B = 2."""
    import dmesh_renderer_amd as dmr
    d, B, H, W, seed = _scene("two_views_ragged")
    ref, gc, gd, rg = _reference(oracle, d, B, H, W, seed)
    t = {k: v.to(hip_device) for k, v in d.items()}
    names = ("verts", "verts_color", "faces_opacity", "verts_depth", "faces_intense")
    leaves = {k: t[k].clone().requires_grad_(True) for k in names}
    r = dmr.TetRenderer(dmr.TetRenderSettings(H, W, t["bg"], seed), full_grads=True)
    color, depth, _ = r(leaves["verts"], t["faces"], leaves["verts_color"], leaves["faces_opacity"], t["mv_mats"], t["proj_mats"],
                        leaves["verts_depth"], leaves["faces_intense"], t["tets"], t["face_tets"], t["tet_faces"])
    th.autograd.backward([color, depth], [gc.to(hip_device), gd.to(hip_device)])
    assert leaves["verts_depth"].grad is None
    assert rel_err(leaves["verts"].grad.cpu().numpy(), rg["verts"]) <= VERTS_TOL
    assert rel_err(leaves["faces_intense"].grad.cpu().numpy(), rg["faces_intense"]) <= FINT_TOL
    assert rel_err(leaves["verts_color"].grad.cpu().numpy(), rg["verts_color"]) <= 1e-4


def test_full_grads_step_replays_as_graph(hip_device):
    """One forward + full-gradient backward captured with torch.cuda.graph matches the eager call."""
    from dmesh_renderer_amd import _C
    d, B, H, W, seed = _scene("small", W_extra=16 * 12)
    args = c_args(d, hip_device, tet=True)
    gc, gd = upstream_grads(B, H, W)
    gcd, gdd = gc.to(hip_device), gd.to(hip_device)

    def step():
        out = _C.render_tets(*args, H, W, seed)
        return _C.render_tets_backward(*args, gcd, gdd, *out[3:7], full_grads=True)

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
from tet_grad_ref import TetGradRef
from util import upstream_grads
O.build()
dev = th.device("cuda:0")
B, H, W = 2, 120, 200
d = scenes.kuhn_tets(5, B, H, W, seed=0, opacity=(0.05, 0.5))
sc = O.scene_from_module_inputs(d, H, W)
_, _, _, ost = O.tet_forward(sc)
ref = TetGradRef(d, H, W, ost)
gc, gd = upstream_grads(B, H, W)
m = ref.mask(); gc, gd = gc * m, gd * m
rg, _, _ = ref.grads(gc, gd)
og = O.tet_backward(sc, ost, gc.numpy(), gd.numpy())
args = c_args(d, dev, tet=True)
for call in range(2):  # re-marching kernel, then the sequence kernel
    out = _C.render_tets(*args, H, W, 0)
    g = [x.cpu().numpy() for x in _C.render_tets_backward(*args, gc.to(dev), gd.to(dev), *out[3:7], full_grads=True)]
    assert rel_err(g[0], rg["verts"]) <= %r, (call, "verts")
    assert rel_err(g[3], rg["faces_intense"]) <= %r, (call, "faces_intense")
    assert rel_err(g[1], og["verts_color"]) <= 1e-4 and rel_err(g[2], og["faces_opacity"]) <= 1e-4, call
print("full fallback ok")
"""


def test_full_grads_direct_atomic_fallback(hip_device):
    """All 20 values per (pixel, face) through the direct atomics: the ablation build with DMR_ABLATE=2048 refuses odd
    faces a table slot (as tests/test_fallback_gpu.py does for the default gradients)."""
    from dmesh_renderer_amd import build
    lib = build.build(ablation=True)
    env = dict(os.environ, DMR_ABLATE="2048", DMR_LIBRARY=lib)
    r = subprocess.run([sys.executable, "-c", FALLBACK_CHILD % (ROOT, HERE, VERTS_TOL, FINT_TOL)], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and "full fallback ok" in r.stdout, r.stdout + r.stderr


def test_two_ranks_full_grads_match_single_rank(hip_device):
    """ShardedTetRenderer(full_grads=True) on two ranks (gloo, one GPU) against TetRenderer(full_grads=True) alone."""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29537", os.path.join(HERE, "sharded_full_grads_child.py")]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=400)
    assert r.returncode == 0 and "sharded full grads ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
