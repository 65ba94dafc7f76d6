"""Child of harness.run_ablation_child: `python tests/fallback_child.py <case>` runs on the ABLATION build of the library
with DMR_ABLATE set to 2048 -- the aggregation tables of the backward kernels (LDS hash tables in front of the global atomics)
refuse rows with an odd id a slot, so those rows take the direct atomics -- and checks the gradients against the oracle
and the float64 models.  --list prints the case names."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import numpy as np
import torch as th

from dmesh_renderer_amd import scenes
from dmesh_renderer_amd.scenes import c_args, rel_err, upstream_grads
from grad_cases import FINT_TOL, MATS_TOL, TET_VERTS_TOL, TRI_VERTS_TOL, module_mats, reference, scene, setup

DEV = th.device("cuda:0")
TRI_NAMES = ("verts", "verts_color", "faces_opacity", "verts_depth", "faces_intense")


def default(_C, O):
    """The default gradients of both renderers (tests/test_fallback_gpu.py)."""
    B, H, W = 2, 200, 328
    d = scenes.layered_sheets(3, 12, B, H, W, seed=0)
    gc, gd = upstream_grads(B, H, W)
    args = c_args(d, DEV)
    out = _C.render_tris(*args, H, W)
    g = _C.render_tris_backward(*args, gc.to(DEV), gd.to(DEV), out[0], *out[3:7])
    sc = O.scene_from_module_inputs(d, H, W)
    _, _, ost = O.tri_forward(sc)
    og = O.tri_backward(sc, ost, gc.numpy(), gd.numpy())
    for t, k in zip(g, TRI_NAMES):
        assert rel_err(t.cpu().numpy(), og[k]) <= 1e-4, k
    d = scenes.kuhn_tets(5, 2, 120, 200)
    gc, gd = upstream_grads(2, 120, 200)
    args = c_args(d, DEV, tet=True)
    out = _C.render_tets(*args, 120, 200, 0)
    g = _C.render_tets_backward(*args, gc.to(DEV), gd.to(DEV), *out[3:7])
    sc = O.scene_from_module_inputs(d, 120, 200)
    _, _, _, ost = O.tet_forward(sc)
    og = O.tet_backward(sc, ost, gc.numpy(), gd.numpy())
    for t, k in zip(g, ("verts_color", "faces_opacity")):
        assert rel_err(t.cpu().numpy(), og[k]) <= 1e-4, k


def tri_exact(_C, O):
    """The exact rows of the tri backward, with exact_grads and with camera_grads (tests/test_tri_exact_grads_gpu.py)."""
    d, B, H, W, _, gc, gd, rg = setup(O, "one_view")
    sc = O.scene_from_module_inputs(d, H, W)
    _, _, ost = O.tri_forward(sc)
    og = O.tri_backward(sc, ost, gc.numpy(), gd.numpy())
    args = c_args(d, DEV)
    for call in range(2):
        out = _C.render_tris(*args, H, W)
        for kw in ({"exact_grads": True}, {"camera_grads": True}):
            g = [x.cpu().numpy() for x in _C.render_tris_backward(*args, gc.to(DEV), gd.to(DEV), out[0], *out[3:7], **kw)]
            assert rel_err(g[0], rg["verts"]) <= TRI_VERTS_TOL, (call, kw, rel_err(g[0], rg["verts"]))
            for i, k in enumerate(TRI_NAMES[1:]):
                assert rel_err(g[1 + i], og[k]) <= 1e-4, (call, kw, k)
        assert np.abs(g[5][:, 3, :3].sum(0) + g[0].sum(0)).max() <= 1e-4 * float(np.abs(g[0]).sum()), call


def tet_full(_C, O):
    """All 20 values per (pixel, face) of the full tet gradients (tests/test_tet_full_grads_gpu.py)."""
    d, B, H, W, seed = scene("two_views_ragged")
    _, gc, gd, rg = reference(O, d, B, H, W, seed)
    sc = O.scene_from_module_inputs(d, H, W)
    _, _, _, ost = O.tet_forward(sc)
    og = O.tet_backward(sc, ost, gc.numpy(), gd.numpy())
    args = c_args(d, DEV, tet=True)
    for call in range(2):  # re-marching kernel, then the sequence kernel
        out = _C.render_tets(*args, H, W, seed)
        g = [x.cpu().numpy() for x in _C.render_tets_backward(*args, gc.to(DEV), gd.to(DEV), *out[3:7], full_grads=True)]
        assert rel_err(g[0], rg["verts"]) <= TET_VERTS_TOL, (call, "verts")
        assert rel_err(g[3], rg["faces_intense"]) <= FINT_TOL, (call, "faces_intense")
        assert rel_err(g[1], og["verts_color"]) <= 1e-4 and rel_err(g[2], og["faces_opacity"]) <= 1e-4, call


def tet_camera(_C, O):
    """The camera variant of the tet backward (tests/test_tet_camera_grads_gpu.py), on a frame 32 columns wider."""
    d, B, H, W, seed = scene("two_views_ragged", W_extra=32)
    _, gc, gd, rg = reference(O, d, B, H, W, seed, camera=True)
    args = c_args(d, DEV, tet=True)
    for call in range(2):  # re-marching kernel, then the sequence kernel
        out = _C.render_tets(*args, H, W, seed)
        g = _C.render_tets_backward(*args, gc.to(DEV), gd.to(DEV), *out[3:7], camera_grads=True)
        g_mv, g_proj = module_mats(args, g)
        assert rel_err(g_mv, rg["mv_mats"]) <= MATS_TOL, (call, "mv")
        assert rel_err(g_proj, rg["proj_mats"]) <= MATS_TOL, (call, "proj")
        assert rel_err(g[0].cpu().numpy(), rg["verts"]) <= 1e-3, (call, "verts")
        assert rel_err(g[1].cpu().numpy(), rg["verts_color"]) <= 1e-4, (call, "verts_color")


CASES = {  # name: (the case, the line printed when it got through)
    "default": (default, "fallback ok"),
    "tri_exact": (tri_exact, "exact fallback ok"),
    "tet_full": (tet_full, "full fallback ok"),
    "tet_camera": (tet_camera, "camera fallback ok"),
}

if __name__ == "__main__":
    if sys.argv[1:] == ["--list"]:
        print(" ".join(CASES))
        sys.exit(0)
    from dmesh_renderer_amd import _C
    from oracle import oracle as O
    O.build()
    run, ok_line = CASES[sys.argv[1]]
    run(_C, O)
    print(ok_line)
