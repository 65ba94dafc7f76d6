"""The fused surface frame (fragments.surface_packed_fused, csrc/dmr_surface.hip) on a scenes.CONFIGS scene (default C4,
fragments=4): hit point, normal towards the camera and mirrored view ray of every packed row, forward + backward.
  default    steps of: one forward + backward of surface_packed_fused and of interpolate_packed_fused(verts) (C = 3) on the same
             lists -- for a kernel trace, so that the new kernels stand next to k_interpolate_packed and
             k_interpolate_packed_backward of the same run.
  --kernels  untraced: the device time by events of the forward, of the backward for all three gradients and for each alone, and
             of the two interpolate calls, with the bytes each moves by construction per second.
  --compare  untraced: three alternating runs of one forward + backward against surface_packed on the device (wall time, peak
             torch.cuda.max_memory_allocated above the inputs), and dL_dverts / dL_dorigin of both against float64 torch on the
             device at the workload's own N."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import torch as th
import dmesh_renderer_amd as dmr
from dmesh_renderer_amd import Fragments, _C, scenes
from dmesh_renderer_amd import fragments as FG

ap = argparse.ArgumentParser(); ap.add_argument("--config", default="C4"); ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--fragments", type=int, default=4); ap.add_argument("--torch-steps", type=int, default=1)
ap.add_argument("--compare", action="store_true"); ap.add_argument("--kernels", action="store_true")
a = ap.parse_args()
dev = th.device("cuda:0")
cfg = scenes.CONFIGS[a.config]
B, H, W, K = cfg.B, cfg.H, cfg.W, a.fragments
t = {k: v.to(dev) for k, v in scenes.make(a.config).items()}
renderer = dmr.TriRenderer(dmr.TriRenderSettings(H, W, t["bg"]), return_fragments=K)
names = ("verts", "faces", "verts_color", "faces_opacity", "mv_mats", "proj_mats", "verts_depth", "faces_intense")
faces = t["faces"].to(th.int32)
F, P = int(faces.shape[0]), int(t["verts"].shape[0])
with th.no_grad():
    frag = renderer(*(t[k] for k in names))[-1]
    face, bary = frag.pix_to_face, frag.bary.contiguous()
    packed = FG.pack_slots_fused(Fragments(face, None, None), F)
    origin = FG.camera_origins(t["mv_mats"]).contiguous()
N = packed.rows
gen = th.Generator(device=dev).manual_seed(2)
ups = [th.randn(N, 3, generator=gen, device=dev) for _ in range(3)]
res = {"config": a.config, "fragments": K, "rows": N, "slots": int(face.numel()), "F": F, "P": P, "B": B, "library": os.path.relpath(_C.library_path(), ROOT)}   # (relative to the repository: the record says which build, not where it lay)
lists = (face, bary, packed.row, packed.n_used, faces)


def device_ms(call, steps):
    ev = [th.cuda.Event(enable_timing=True) for _ in range(2)]
    for i in range(3 + steps):
        if i == 3: ev[0].record()
        call()
    ev[1].record(); th.cuda.synchronize()
    return round(ev[0].elapsed_time(ev[1]) / steps, 4)


def timed(fn, steps, warm=1):
    for _ in range(warm):
        fn()
    th.cuda.synchronize(); base = th.cuda.memory_allocated(); th.cuda.reset_peak_memory_stats(); t0 = time.perf_counter()
    for _ in range(steps):
        out = fn()
    th.cuda.synchronize(); dt = (time.perf_counter() - t0) / steps
    return round(dt * 1e3, 3), round((th.cuda.max_memory_allocated() - base) / 2**20, 1), out


def step(fn, dtype=th.float32):
    lv = [x.to(dtype).clone().requires_grad_(True) for x in (t["verts"], bary, origin)]
    s = fn(Fragments(face, lv[1], None), packed, faces, lv[0], lv[2])
    return th.autograd.grad(list(s), lv, grad_outputs=[u.to(dtype) for u in ups])


if not (a.compare or a.kernels):
    for _ in range(3 + a.steps):
        step(FG.surface_packed_fused)
        v = t["verts"].clone().requires_grad_(True)
        b = bary.clone().requires_grad_(True)
        x = FG.interpolate_packed_fused(Fragments(face, b, None), packed, faces, v)
        th.autograd.grad(x, [v, b], grad_outputs=ups[0])
    th.cuda.synchronize()
    print(json.dumps(res)); sys.exit(0)
if a.kernels:
    lists_bytes = int(face.numel()) * (4 + 4 + 8)   # face, row, bary of every slot
    k = {"k_surface_packed": device_ms(lambda: _C.surface_packed(*lists, t["verts"], origin, N), a.steps)}
    for label, need in (("all three gradients", (True, True, True)), ("dL_dverts alone", (True, False, False)), ("dL_dbary alone", (False, True, False)),
                        ("dL_dorigin alone", (False, False, True)), ("dL_dbary and dL_dorigin", (False, True, True))):
        k["backward, " + label + " (fills + k_surface_packed_backward)"] = device_ms(lambda: _C.surface_packed_backward(*lists, t["verts"], origin, *ups, need), a.steps)
    k["backward, all three gradients, grad_hit alone"] = device_ms(lambda: _C.surface_packed_backward(*lists, t["verts"], origin, ups[0], None, None, (True, True, True)), a.steps)
    k["k_interpolate_packed (C = 3)"] = device_ms(lambda: _C.interpolate_packed(*lists, t["verts"], N), a.steps)
    k["interpolate_packed_backward (C = 3, zero + kernel)"] = device_ms(lambda: _C.interpolate_packed_backward(*lists, t["verts"], ups[0], (True, True)), a.steps)
    res["ms"] = k
    res["forward_bytes"] = N * 36 + lists_bytes
    res["backward_bytes"] = N * 36 + lists_bytes + int(face.numel()) * 8 + 2 * 12 * P
    res["forward_TB_per_s"] = round(res["forward_bytes"] / (k["k_surface_packed"] * 1e-3) / 1e12, 3)
    res["backward_TB_per_s"] = round(res["backward_bytes"] / (k["backward, all three gradients (fills + k_surface_packed_backward)"] * 1e-3) / 1e12, 3)
    res["interpolate_forward_TB_per_s"] = round((N * 12 + lists_bytes) / (k["k_interpolate_packed (C = 3)"] * 1e-3) / 1e12, 3)
    print(json.dumps(res)); sys.exit(0)
# --compare
res["runs"] = []
for _ in range(3):
    r = {}
    r["torch_ms"], r["torch_peak_MiB"], gt = timed(lambda: step(FG.surface_packed), a.torch_steps)
    r["fused_ms"], r["fused_peak_MiB"], gf = timed(lambda: step(FG.surface_packed_fused), a.steps)
    r["time_ratio"], r["memory_ratio"] = round(r["torch_ms"] / r["fused_ms"], 3), round(r["torch_peak_MiB"] / max(r["fused_peak_MiB"], 0.1), 3)
    res["runs"].append(r)
g64 = step(FG.surface_packed, th.float64)
rel = lambda x, ref: float((x.double() - ref).abs().max() / ref.abs().max())
res["against_float64_torch"] = {n: {"fused": rel(gf[i], g64[i]), "float32_torch": rel(gt[i], g64[i]), "max_abs_ref": float(g64[i].abs().max())}
                                for i, n in ((0, "dL_dverts"), (1, "dL_dbary"), (2, "dL_dorigin"))}
print(json.dumps(res))
