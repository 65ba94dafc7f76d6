"""fragments.face_visibility_fused on a scenes.CONFIGS tri scene's fragment lists (default C4, fragments=4): every step renders
the lists (k_tri_fragments), composites verts_color over them (k_composite_fragments, C = 3: the kernel to read the forward's
time against) and runs one fused visibility forward + backward with coverage=True, a pixel_weight, gradients to faces_opacity
and pixel_weight.  --compare also times one forward + backward of fragments.face_visibility + face_coverage (plain torch) on
the same lists, and reports both paths' wall time and peak memory above what the inputs hold (torch.cuda.max_memory_allocated)."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import torch as th
from dmesh_renderer_amd import Fragments, _C, scenes
from dmesh_renderer_amd import fragments as FG

ap = argparse.ArgumentParser(); ap.add_argument("--config", default="C4"); ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--fragments", type=int, default=4)
ap.add_argument("--compare", action="store_true", help="also the torch path, with wall time and peak memory of both")
a = ap.parse_args()
dev = th.device("cuda:0")
cfg = scenes.CONFIGS[a.config]
B, H, W, K = cfg.B, cfg.H, cfg.W, a.fragments
d = scenes.make(a.config)
args = scenes.c_args(d, dev)
faces = d["faces"].to(dev).to(th.int32)
F = int(faces.shape[0])
gen = th.Generator().manual_seed(3)
colour = d["verts_color"].to(dev)
opacity = d["faces_opacity"].to(dev).requires_grad_(True)
weight = th.randn(B, H, W, generator=gen).to(dev).requires_grad_(True)
g_vis = th.randn(B, F, generator=gen).to(dev)

def lists():
    o = _C.render_tris(*args, H, W, fragments=K)
    return Fragments(o[7], o[8], o[9])

def fused(frag):
    vis, max_weight, pixels = FG.face_visibility_fused(frag, opacity, F, weight, coverage=True)
    return (vis, max_weight, pixels) + th.autograd.grad((vis * g_vis).sum(), [opacity, weight])

def torch_path(frag):
    vis = FG.face_visibility(frag, opacity, F, weight)
    max_weight, pixels = FG.face_coverage(frag, opacity, F)
    return (vis, max_weight, pixels) + th.autograd.grad((vis * g_vis).sum(), [opacity, weight])

def timed(fn, steps, render):
    frag = lists()
    for _ in range(3):
        if render: FG.composite_fused(lists(), faces, opacity.detach(), colour)
        fn(lists() if render else frag)
    th.cuda.synchronize(); base = th.cuda.memory_allocated(); th.cuda.reset_peak_memory_stats(); t0 = time.perf_counter()
    for _ in range(steps):
        f = lists() if render else frag
        if render: FG.composite_fused(f, faces, opacity.detach(), colour)
        out = fn(f)
    th.cuda.synchronize(); dt = (time.perf_counter() - t0) / steps
    return round(dt * 1e3, 4), round((th.cuda.max_memory_allocated() - base) / 2**20, 1), out

res = {"config": a.config, "fragments": K, "image": [H, W], "views": B, "faces": F}
res["fused_with_render_and_composite_ms"], _, _ = timed(fused, a.steps, True)
if a.compare:
    res["fused_ms"], res["fused_peak_MiB"], gf = timed(fused, a.steps, False)
    res["torch_ms"], res["torch_peak_MiB"], gt = timed(torch_path, max(2, a.steps // 4), False)
    res["time_ratio"] = round(res["torch_ms"] / res["fused_ms"], 2)
    res["memory_ratio"] = round(res["torch_peak_MiB"] / max(res["fused_peak_MiB"], 0.1), 2)
    for cov in (True, False):  # the forward alone, with and without the maximum and the count (device time by events, no autograd)
        frag, ev = lists(), [th.cuda.Event(enable_timing=True) for _ in range(2)]
        with th.no_grad():
            for i in range(3 + a.steps):
                if i == 3: ev[0].record()
                FG.face_visibility_fused(frag, opacity, F, weight, coverage=cov)
        ev[1].record(); th.cuda.synchronize()
        res["forward_coverage_ms" if cov else "forward_no_coverage_ms"] = round(ev[0].elapsed_time(ev[1]) / a.steps, 4)
    names = ("vis", "max_weight", "pixels", "dL_dfaces_opacity", "dL_dpixel_weight")
    res["rel_err_fused_vs_torch"] = {n: float(scenes.rel_err(x.detach().double().cpu().numpy(), y.detach().double().cpu().numpy())) for n, x, y in zip(names, gf, gt)}
print(json.dumps(res))
