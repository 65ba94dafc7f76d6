"""Child of harness.run_ranks: `sharded_child.py <case>` is one rank of a 2-rank (gloo) run of the sharded Modules on one
GPU.  Every rank also renders the full image alone and compares: the images bit for bit, the gradients to GRAD_TOL.
--list prints the case names."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import numpy as np
import torch as th
import torch.distributed as dist

import dmesh_renderer_amd as dmr
from dmesh_renderer_amd import scenes, sharding
from harness import module_step
from util import with_bg

DEV = th.device("cuda:0")
GRAD_TOL = 1e-5
TRI_NAMES = ("verts", "verts_color", "faces_opacity", "verts_depth", "faces_intense")


def compare(full, sharded, names, tol, what):
    """(images, gradients) of module_step, unsharded and sharded; `tol` is a bound or a function of the gradient's name."""
    for a, b in zip(sharded[0], full[0]):
        assert th.equal(a, b), (what, "image differs")
    for k in names:
        e = scenes.rel_err(sharded[1][k].cpu().numpy(), full[1][k].cpu().numpy())
        assert e <= (tol(k) if callable(tol) else tol), (what, k, e)


def on_device(d, B, H, W, alpha=False):
    """The scene over util.BG and the upstream gradients (g_c, g_d[, g_a]) on the device, and the renderer's settings.  (A
    band's image is zero outside its rows, not background: the assembled images are still compared bit for bit.)"""
    t = {k: v.to(DEV) for k, v in with_bg(d).items()}
    up = list(scenes.upstream_grads(B, H, W))
    if alpha:
        up.append(th.randn(B, 1, H, W, generator=th.Generator().manual_seed(5)))
    settings = dmr.TetRenderSettings(H, W, t["bg"], 0) if "tets" in t else dmr.TriRenderSettings(H, W, t["bg"])
    return t, [x.to(DEV) for x in up], settings


def sharded_vs_full(d, B, H, W, names, **kw):
    """The scene `d` through the Module alone and through the assembling sharded Module (tri: both partitions), both
    made with the keywords `kw`, compared -> the unsharded outputs."""
    tet = "tets" in d
    t, up, settings = on_device(d, B, H, W, alpha=kw.get("return_alpha", False))
    full = module_step((dmr.TetRenderer if tet else dmr.TriRenderer)(settings, **kw), t, names, up)
    for part in ({},) if tet else ({"partition": "bands"}, {"partition": "view_bands"}):
        sh = (sharding.ShardedTetRenderer if tet else sharding.ShardedTriRenderer)(settings, assemble=True, **part, **kw)
        assert sh.world == dist.get_world_size() == 2 and (not tet or sh.rows != (0, 0))
        compare(full, module_step(sh, t, names, up), names, GRAD_TOL, (part, kw))
    return full[0]


def base():
    """ShardedTriRenderer, assembled or not: bands of both views per rank / (view, band) segments (B = 2 views, 2 ranks);
    then ShardedTetRenderer (bands, one all-gather of the images, ONE all-reduce over [3P | F])."""
    rank = dist.get_rank()
    B, H, W = 2, 200, 328
    t, up, settings = on_device(scenes.layered_sheets(3, 14, B, H, W, seed=9), B, H, W)
    full = module_step(dmr.TriRenderer(settings), t, TRI_NAMES, up)
    for partition in ("bands", "view_bands"):
        for assemble in (True, False):
            sh = sharding.ShardedTriRenderer(settings, assemble=assemble, partition=partition)
            assert sh.world == dist.get_world_size() == 2 and sh.rows != (0, 0)
            if partition == "view_bands":  # the second view costs twice the first: rank 0 renders view 0 and the top of view 1
                gy = sharding.tile_rows(H)
                sh.set_row_work(np.stack([np.ones(gy), 2.0 * np.ones(gy)]))
                sh.segment_cost_per_face = 0.0
                parts = sh.view_parts(B, t["faces"].shape[0])
                assert [len(p) for p in parts] == [2, 1], parts
            if assemble:
                mine = lambda im: im
            elif partition == "bands":       # this rank's band rows of the colour image
                r0, r1 = sh.rows
                mine = lambda im: [im[0][:, :, 16 * r0:16 * r1]]
            else:                            # this rank's segments of it
                mine = lambda im: [im[0][v, :, 16 * r0:16 * r1] for v, r0, r1 in parts[rank]]
            im, g = module_step(sh, t, TRI_NAMES, up)
            compare((mine(full[0]), full[1]), (mine(im), g), TRI_NAMES, scenes.sum_order_tol, (partition, assemble))
    out = sharded_vs_full(scenes.kuhn_tets(5, B, 160, 160, seed=3), B, 160, 160, ("verts_color", "faces_opacity"))
    assert bool(out[2].any())


def full_grads():
    sharded_vs_full(scenes.kuhn_tets(5, 2, 160, 160, seed=3), 2, 160, 160,
                    ("verts", "verts_color", "faces_opacity", "faces_intense"), full_grads=True)


def exact_grads():
    sharded_vs_full(scenes.layered_sheets(3, 9, 2, 96, 160, seed=4), 2, 96, 160,
                    ("verts", "verts_color", "faces_opacity", "mv_mats", "proj_mats", "verts_depth", "faces_intense"), camera_grads=True)


def camera_grads_tet():
    sharded_vs_full(scenes.kuhn_tets(5, 2, 160, 176, seed=3), 2, 160, 176,
                    ("verts", "verts_color", "faces_opacity", "mv_mats", "proj_mats", "faces_intense"), camera_grads=True)


def alpha():
    B, H, W = 2, 96, 176
    out = sharded_vs_full(scenes.layered_sheets(3, 9, B, H, W, seed=4), B, H, W, TRI_NAMES, return_alpha=True)
    assert float(out[2].max()) > 0.3
    out = sharded_vs_full(scenes.kuhn_tets(4, B, H, W, seed=3), B, H, W, ("verts_color", "faces_opacity"), return_alpha=True)
    assert float(out[3].max()) > 0.05


CASES = {  # name: (the case, the line rank 0 prints when every rank got through it)
    "base": (base, "sharded ok"),
    "full_grads": (full_grads, "sharded full grads ok"),
    "exact_grads": (exact_grads, "sharded exact grads ok"),
    "camera_grads_tet": (camera_grads_tet, "sharded camera grads ok"),
    "alpha": (alpha, "sharded alpha ok"),
}

if __name__ == "__main__":
    if sys.argv[1:] == ["--list"]:
        print(" ".join(CASES))
        sys.exit(0)
    run, ok_line = CASES[sys.argv[1]]
    dist.init_process_group(backend="gloo")
    th.cuda.set_device(DEV)
    run()
    dist.barrier()
    if dist.get_rank() == 0:
        print(ok_line)
    dist.destroy_process_group()
