"""fragments.composite_fused on a scenes.CONFIGS tri scene's fragment lists (default C4, fragments=4): every step renders the
lists (k_tri_fragments) and runs one fused forward + backward over them with C channels (C = 3: verts_color; else N(0, 1)
attributes), face_scale = faces_intense, gradients to faces_opacity, vert_attrs and face_scale (--bary: to the lists'
barycentrics too).  --compare also times one forward + backward of fragments.composite (plain torch) on the same lists, and
reports both paths' wall time and peak memory above what the inputs hold (torch.cuda.max_memory_allocated)."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import torch as th
from dmesh_renderer_amd import Fragments, _C, scenes
from dmesh_renderer_amd import fragments as FG

ap = argparse.ArgumentParser(); ap.add_argument("--config", default="C4"); ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--fragments", type=int, default=4); ap.add_argument("--channels", type=int, default=3)
ap.add_argument("--bary", action="store_true", help="also the gradient of the barycentrics")
ap.add_argument("--compare", action="store_true", help="also fragments.composite, with wall time and peak memory of both")
a = ap.parse_args()
dev = th.device("cuda:0")
cfg = scenes.CONFIGS[a.config]
B, H, W, K, C = cfg.B, cfg.H, cfg.W, a.fragments, a.channels
d = scenes.make(a.config)
args = scenes.c_args(d, dev)
faces = d["faces"].to(dev).to(th.int32)
gen = th.Generator().manual_seed(3)
attrs = (d["verts_color"] if C == 3 else th.randn(d["verts"].shape[0], C, generator=gen)).to(dev).requires_grad_(True)
opacity = d["faces_opacity"].to(dev).requires_grad_(True)
scale = d["faces_intense"].to(dev).requires_grad_(True)
g_image, g_T = th.randn(B, C, H, W, generator=gen).to(dev), th.randn(B, 1, H, W, generator=gen).to(dev)
leaves = [opacity, attrs, scale]

def lists():
    o = _C.render_tris(*args, H, W, fragments=K)
    bary = o[8].requires_grad_(True) if a.bary else o[8]
    return Fragments(o[7], bary, o[9])

def shade(fn, frag):
    image, T = fn(frag, faces, opacity, attrs, face_scale=scale)
    return th.autograd.grad((image * g_image).sum() + (T * g_T).sum(), leaves + ([frag.bary] if a.bary else []))

def timed(fn, steps, render):
    frag = lists()
    for _ in range(3): shade(fn, lists() if render else frag)
    th.cuda.synchronize(); base = th.cuda.memory_allocated(); th.cuda.reset_peak_memory_stats(); t0 = time.perf_counter()
    for _ in range(steps): g = shade(fn, lists() if render else frag)
    th.cuda.synchronize(); dt = (time.perf_counter() - t0) / steps
    return round(dt * 1e3, 4), round((th.cuda.max_memory_allocated() - base) / 2**20, 1), g

res = {"config": a.config, "fragments": K, "channels": C, "bary": a.bary, "image": [H, W], "faces": int(faces.shape[0])}
res["fused_with_render_ms"], _, _ = timed(FG.composite_fused, a.steps, True)
if a.compare:
    res["fused_ms"], res["fused_peak_MiB"], gf = timed(FG.composite_fused, a.steps, False)
    res["torch_ms"], res["torch_peak_MiB"], gt = timed(FG.composite, max(2, a.steps // 4), False)
    res["time_ratio"] = round(res["torch_ms"] / res["fused_ms"], 2)
    res["memory_ratio"] = round(res["torch_peak_MiB"] / max(res["fused_peak_MiB"], 0.1), 2)
    res["grad_rel_err"] = [float(scenes.rel_err(x.cpu().numpy(), y.cpu().numpy())) for x, y in zip(gf, gt)]
print(json.dumps(res))
