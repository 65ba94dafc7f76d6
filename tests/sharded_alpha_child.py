"""Child of tests/test_alpha_gpu.py: one rank of a 2-rank (gloo) run of ShardedTriRenderer (both partitions) and
ShardedTetRenderer with return_alpha=True on one GPU.  Every rank also renders the full image alone and compares."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import torch as th
import torch.distributed as dist
import dmesh_renderer_amd as dmr
from dmesh_renderer_amd import scenes, sharding

dist.init_process_group(backend="gloo")
rank, world = dist.get_rank(), dist.get_world_size()
dev = th.device("cuda:0")
th.cuda.set_device(dev)
B, H, W = 2, 96, 176
gc, gd = scenes.upstream_grads(B, H, W)
ga = th.randn(B, 1, H, W, generator=th.Generator().manual_seed(5))
gc, gd, ga = gc.to(dev), gd.to(dev), ga.to(dev)

d = scenes.layered_sheets(3, 9, B, H, W, seed=4)
t = {k: v.to(dev) for k, v in d.items()}
settings = dmr.TriRenderSettings(H, W, t["bg"])
names = ("verts", "verts_color", "faces_opacity", "verts_depth", "faces_intense")


def run_tri(renderer):
    leaves = {k: t[k].clone().requires_grad_(True) for k in names}
    color, depth, alpha = renderer(leaves["verts"], t["faces"], leaves["verts_color"], leaves["faces_opacity"], t["mv_mats"],
                                   t["proj_mats"], leaves["verts_depth"], leaves["faces_intense"])
    th.autograd.backward([color, depth, alpha], [gc, gd, ga])
    return [color.detach(), depth.detach(), alpha.detach()], [leaves[k].grad for k in names]


full = run_tri(dmr.TriRenderer(settings, return_alpha=True))
assert float(full[0][2].max()) > 0.3
for partition in ("bands", "view_bands"):
    sh = sharding.ShardedTriRenderer(settings, assemble=True, partition=partition, return_alpha=True)
    assert sh.world == world == 2
    im, g = run_tri(sh)
    for a, b in zip(im, full[0]):
        assert th.equal(a, b), (partition, "assembled tri image differs")
    for a, b, k in zip(g, full[1], names):
        e = scenes.rel_err(a.cpu().numpy(), b.cpu().numpy())
        assert e <= 1e-5, (partition, k, e)

d = scenes.kuhn_tets(4, B, H, W, seed=3)
t = {k: v.to(dev) for k, v in d.items()}
tsettings = dmr.TetRenderSettings(H, W, t["bg"], 0)
tnames = ("verts_color", "faces_opacity")


def run_tet(renderer):
    leaves = {k: t[k].clone().requires_grad_(True) for k in tnames}
    color, depth, active, alpha = renderer(t["verts"], t["faces"], leaves["verts_color"], leaves["faces_opacity"], t["mv_mats"],
                                           t["proj_mats"], t["verts_depth"], t["faces_intense"], t["tets"], t["face_tets"], t["tet_faces"])
    th.autograd.backward([color, depth, alpha], [gc, gd, ga])
    return [color.detach(), depth.detach(), active, alpha.detach()], [leaves[k].grad for k in tnames]


full = run_tet(dmr.TetRenderer(tsettings, return_alpha=True))
assert float(full[0][3].max()) > 0.05
sh = sharding.ShardedTetRenderer(tsettings, assemble=True, return_alpha=True)
assert sh.world == world == 2 and sh.rows != (0, 0)
im, g = run_tet(sh)
for a, b in zip(im, full[0]):
    assert th.equal(a, b), "assembled tet image differs"
for a, b, k in zip(g, full[1], tnames):
    e = scenes.rel_err(a.cpu().numpy(), b.cpu().numpy())
    assert e <= 1e-5, (k, e)
dist.barrier()
if rank == 0:
    print("sharded alpha ok")
dist.destroy_process_group()
