"""fragments.interpolate_fused + composite_values_fused on a scenes.CONFIGS tri scene's fragment lists (default C4, fragments=4):
every step renders the lists (k_tri_fragments), composites C channels of per-vertex attributes over them with composite_fused
(k_composite_fragments + k_composite_fragments_backward: the kernels to read the new ones' times against) and runs the deferred
chain forward + backward: interpolate_fused, a pointwise torch op on every fragment, composite_values_fused, gradients to
vert_attrs, bary, faces_opacity and face_scale (and through values).  --compare also times one forward + backward of the torch
path (fragments.interpolate + composite_values) on the same lists, and reports both paths' wall time and peak memory above what
the inputs hold (torch.cuda.max_memory_allocated), and each new kernel's device time by events with the bytes it moves by
construction (4 B K C H W for both forwards and for the dL/dvalues store)."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import torch as th
from dmesh_renderer_amd import Fragments, _C, scenes
from dmesh_renderer_amd import fragments as FG

ap = argparse.ArgumentParser(); ap.add_argument("--config", default="C4"); ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--fragments", type=int, default=4); ap.add_argument("--channels", type=int, default=3)
ap.add_argument("--compare", action="store_true", help="also the torch path, with wall time and peak memory of both, and per-kernel bytes/s")
a = ap.parse_args()
dev = th.device("cuda:0")
cfg = scenes.CONFIGS[a.config]
B, H, W, K, C = cfg.B, cfg.H, cfg.W, a.fragments, a.channels
d = scenes.make(a.config)
args = scenes.c_args(d, dev)
faces = d["faces"].to(dev).to(th.int32)
F, P = int(faces.shape[0]), int(d["verts"].shape[0])
gen = th.Generator().manual_seed(3)
attrs = th.randn(P, C, generator=gen).to(dev).requires_grad_(True)
opacity = d["faces_opacity"].to(dev).requires_grad_(True)
scale = (th.rand(B, F, generator=gen) + 0.5).to(dev).requires_grad_(True)
g_image = th.randn(B, C, H, W, generator=gen).to(dev)
g_T = th.randn(B, 1, H, W, generator=gen).to(dev)
LEAVES = ("vert_attrs", "bary", "faces_opacity", "face_scale")

def lists():
    o = _C.render_tris(*args, H, W, fragments=K)
    return o[7], o[8].requires_grad_(True)

def loss(image, T):
    return (image * g_image).sum() + (T * g_T).sum()

def fused(face, bary):
    a_k = FG.interpolate_fused(Fragments(face, bary, None), faces, attrs)
    image, T = FG.composite_values_fused(Fragments(face, None, None), opacity, th.tanh(a_k), scale)   # (the caller's own shader)
    return (image, T) + th.autograd.grad(loss(image, T), [attrs, bary, opacity, scale])

def torch_path(face, bary):
    a_k = FG.interpolate(Fragments(face, bary, None), faces, attrs)
    image, T = FG.composite_values(Fragments(face, None, None), opacity, th.tanh(a_k), scale)
    return (image, T) + th.autograd.grad(loss(image, T), [attrs, bary, opacity, scale])

def whole_shader(face, bary):
    image, T = FG.composite_fused(Fragments(face, bary, None), faces, opacity, attrs, face_scale=scale)
    return th.autograd.grad(loss(image, T), [attrs, bary, opacity, scale])

def timed(fn, steps, render, warm=3):
    fl = lists()
    for _ in range(warm):
        if render: whole_shader(*lists())
        fn(*(lists() if render else fl))
    th.cuda.synchronize(); base = th.cuda.memory_allocated(); th.cuda.reset_peak_memory_stats(); t0 = time.perf_counter()
    for _ in range(steps):
        f = lists() if render else fl
        if render: whole_shader(*f)
        out = fn(*f)
    th.cuda.synchronize(); dt = (time.perf_counter() - t0) / steps
    return round(dt * 1e3, 4), round((th.cuda.max_memory_allocated() - base) / 2**20, 1), out

def device_ms(call, steps):
    ev = [th.cuda.Event(enable_timing=True) for _ in range(2)]
    for i in range(3 + steps):
        if i == 3: ev[0].record()
        call()
    ev[1].record(); th.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / steps

res = {"config": a.config, "fragments": K, "channels": C, "image": [H, W], "views": B, "faces": F, "verts": P}
res["fused_with_render_and_composite_fused_ms"], _, _ = timed(fused, a.steps, True)
if a.compare:
    res["fused_ms"], res["fused_peak_MiB"], gf = timed(fused, a.steps, False)
    res["torch_ms"], res["torch_peak_MiB"], gt = timed(torch_path, max(2, a.steps // 10), False, warm=1)
    res["time_ratio"] = round(res["torch_ms"] / res["fused_ms"], 2)
    res["memory_ratio"] = round(res["torch_peak_MiB"] / max(res["fused_peak_MiB"], 0.1), 2)
    names = ("image", "T", "dL_dvert_attrs", "dL_dbary", "dL_dfaces_opacity", "dL_dface_scale")
    res["rel_err_fused_vs_torch"] = {n: float(scenes.rel_err(x.detach().double().cpu().numpy(), y.detach().double().cpu().numpy())) for n, x, y in zip(names, gf, gt)}
    # each kernel alone, device time by events (no autograd): bytes by construction = 4 B K C H W
    face, bary = lists()
    bary, at, op, sc = bary.detach(), attrs.detach(), opacity.detach(), scale.detach()
    values = _C.interpolate_fragments(face, bary, faces, at)
    g_out = th.randn(values.shape, generator=th.Generator(device=dev).manual_seed(1), device=dev)
    plane = 4 * B * K * C * H * W
    kern = {
        "k_interpolate_fragments": lambda: _C.interpolate_fragments(face, bary, faces, at),
        "k_composite_values": lambda: _C.composite_values(face, op, values, sc),
        "k_interpolate_fragments_backward": lambda: _C.interpolate_fragments_backward(face, bary, faces, at, g_out, (True, True)),
        "k_composite_values_backward": lambda: _C.composite_values_backward(face, op, values, sc, g_image, g_T, (True, True, True)),
        "k_composite_values_backward, dL_dvalues alone": lambda: _C.composite_values_backward(face, op, values, sc, g_image, None, (False, True, False)),
        "k_composite_fragments": lambda: _C.composite_fragments(face, bary, faces, op, at, sc),
    }
    res["kernels"] = {}
    for n, call in kern.items():
        ms = device_ms(call, a.steps)
        res["kernels"][n] = {"ms": round(ms, 4), "plane_GBps": round(plane / ms / 1e6, 1)}
    res["plane_bytes"] = plane
print(json.dumps(res))
