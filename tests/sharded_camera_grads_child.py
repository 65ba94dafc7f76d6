"""Child of tests/test_tet_camera_grads_gpu.py: one rank of a 2-rank (gloo) run of ShardedTetRenderer(camera_grads=True)
on one GPU.  Every rank also renders the full image alone and compares."""
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
B, H, W = 2, 160, 176
d = scenes.kuhn_tets(5, B, H, W, seed=3)
t = {k: v.to(dev) for k, v in d.items()}
gc, gd = scenes.upstream_grads(B, H, W)
gc, gd = gc.to(dev), gd.to(dev)
settings = dmr.TetRenderSettings(H, W, t["bg"], 0)
names = ("verts", "verts_color", "faces_opacity", "mv_mats", "proj_mats", "faces_intense")


def run(renderer):
    leaves = {k: t[k].clone().requires_grad_(True) for k in names}
    color, depth, active = renderer(leaves["verts"], t["faces"], leaves["verts_color"], leaves["faces_opacity"], leaves["mv_mats"],
                                    leaves["proj_mats"], t["verts_depth"], leaves["faces_intense"], t["tets"], t["face_tets"], t["tet_faces"])
    th.autograd.backward([color, depth], [gc, gd])
    return color.detach(), depth.detach(), [leaves[k].grad for k in names]


full = run(dmr.TetRenderer(settings, camera_grads=True))
sh = sharding.ShardedTetRenderer(settings, assemble=True, camera_grads=True)
assert sh.world == world == 2 and sh.rows != (0, 0)
c, z, g = run(sh)
assert th.equal(c, full[0]) and th.equal(z, full[1]), "assembled tet image differs"
for a, b, k in zip(g, full[2], names):
    e = scenes.rel_err(a.cpu().numpy(), b.cpu().numpy())
    assert e <= 1e-5, (k, e)
dist.barrier()
if rank == 0:
    print("sharded camera grads ok")
dist.destroy_process_group()
