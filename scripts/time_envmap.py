"""The fused environment-map lookup (fragments.envmap_rows_fused / EnvMap, csrc/dmr_envmap.hip) on a scenes.CONFIGS scene (default
C4, fragments=4, C = 3), on two row sets: the BACKGROUND's rows (pixel_directions, N = B H W) and the PACKED rows of the fragment
lists (hit - camera origin, what a specular term looks up), each also randomly permuted ("shuffled").
  default    steps of: one forward + backward of EnvMap(256, 512) on both row sets and of ViewSH(4) on the packed rows -- for a
             kernel trace, so that the new kernels stand next to k_sh_rows and k_sh_rows_backward of the same run.
  --kernels  untraced: the new kernels' device time by events for 256 x 512 and 1024 x 2048 maps on the four row sets (forward;
             backward for both gradients, for dL/dd alone, for dL/denvmap alone), next to k_sh_rows / k_sh_rows_backward on the
             packed rows, with the bytes each moves by construction per second; the forward per C (1, 3, 4, 5, 8, 16).  On the
             ablation build (DMR_LIBRARY) DMR_ABLATE bit 67108864 runs every chunk count's OTHER store shape -- the two runs
             together are the store-shape table --, and bit 134217728 counts the share of dL/denvmap contributions that leave as
             direct atomics.
  --compare  untraced: three alternating runs of EnvMap against envmap_rows on the device (wall time, peak
             torch.cuda.max_memory_allocated above the inputs), and the float32 deviation at 1024 x 2048 (and 512 x 1024) against
             float64 torch on the device."""
import argparse, ctypes, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import torch as th
import dmesh_renderer_amd as dmr
from dmesh_renderer_amd import Fragments, _C, scenes
from dmesh_renderer_amd import fragments as FG

ap = argparse.ArgumentParser(); ap.add_argument("--config", default="C4"); ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--fragments", type=int, default=4); ap.add_argument("--torch-steps", type=int, default=2)
ap.add_argument("--compare", action="store_true"); ap.add_argument("--kernels", action="store_true")
a = ap.parse_args()
dev = th.device("cuda:0")
cfg = scenes.CONFIGS[a.config]
B, H, W, K = cfg.B, cfg.H, cfg.W, a.fragments
t = {k: v.to(dev) for k, v in scenes.make(a.config).items()}
renderer = dmr.TriRenderer(dmr.TriRenderSettings(H, W, t["bg"]), return_fragments=K)
names = ("verts", "faces", "verts_color", "faces_opacity", "mv_mats", "proj_mats", "verts_depth", "faces_intense")
faces = t["faces"].to(th.int32)
F = int(faces.shape[0])
MAPS = ((256, 512), (1024, 2048))
ABLATE = int(os.environ.get("DMR_ABLATE", "0") or 0)


def row_sets():
    """{name: d [N,3]}: the background's pixel directions, the packed rows' view directions, and both shuffled"""
    with th.no_grad():
        frag = renderer(*(t[k] for k in names))[-1]
        lists = Fragments(frag.pix_to_face, None, None)
        packed = FG.pack_slots_fused(lists, F)
        hit = _C.interpolate_packed(frag.pix_to_face, frag.bary, packed.row, packed.n_used, faces, t["verts"], packed.rows)
        view = FG.packed_row_views_fused(lists, packed)
        origin = FG.camera_origins(t["mv_mats"]).contiguous()
        sets = {"background": FG.pixel_directions(t["mv_mats"], t["proj_mats"], H, W).reshape(-1, 3).contiguous(),
                "packed": (hit - origin[view.clamp(min=0).long()]).contiguous()}
        g = th.Generator(device=dev).manual_seed(3)
        for k in ("background", "packed"):
            sets[k + ", shuffled"] = sets[k][th.randperm(sets[k].shape[0], generator=g, device=dev)].contiguous()
    return sets, hit, view, origin


def device_ms(call, steps):
    ev = [th.cuda.Event(enable_timing=True) for _ in range(2)]
    for i in range(3 + steps):
        if i == 3: ev[0].record()
        call()
    ev[1].record(); th.cuda.synchronize()
    return round(ev[0].elapsed_time(ev[1]) / steps, 4)


def timed(fn, steps, args, warm=1):
    for _ in range(warm):
        fn(*args)
    th.cuda.synchronize(); base = th.cuda.memory_allocated(); th.cuda.reset_peak_memory_stats(); t0 = time.perf_counter()
    for _ in range(steps):
        out = fn(*args)
    th.cuda.synchronize(); dt = (time.perf_counter() - t0) / steps
    return round(dt * 1e3, 3), round((th.cuda.max_memory_allocated() - base) / 2**20, 1), out


def stats_of(call):
    """(contributions, direct atomics) of one call, from the ablation build's counters; None on the product library"""
    lib = ctypes.CDLL(_C.library_path())
    fn = getattr(lib, "dmr_envmap_stats", None)
    if fn is None or not ABLATE & (1 << 27):
        return None
    out = (ctypes.c_ulonglong * 2)()
    th.cuda.synchronize(); fn(None, 1); call(); th.cuda.synchronize(); fn(out, 1)
    return {"contributions": int(out[0]), "direct_atomics": int(out[1]), "share": round(out[1] / max(out[0], 1), 5)}


sets, hit, view, origin = row_sets()
res = {"config": a.config, "fragments": K, "rows": {k: int(v.shape[0]) for k, v in sets.items()}, "library": _C.library_path(), "DMR_ABLATE": ABLATE}
gen = th.Generator(device=dev).manual_seed(2)
if not (a.compare or a.kernels):
    env, sh = FG.EnvMap(*MAPS[0]).to(dev), FG.ViewSH(4)
    for _ in range(3 + a.steps):
        for k in ("background", "packed"):
            d = sets[k].clone().requires_grad_(True)
            env(d).sum().backward()
        x = hit.clone().requires_grad_(True)
        sh(x, origin, view).sum().backward()
    th.cuda.synchronize()
    print(json.dumps(res)); sys.exit(0)
if a.kernels:
    C = 3
    res["maps"] = {}
    for He, We in MAPS:
        env = th.randn(He, We, C, generator=gen, device=dev)
        per = {}
        for k, d in sets.items():
            N = int(d.shape[0])
            up = th.randn(N, C, generator=gen, device=dev)
            r = {"k_envmap_rows": device_ms(lambda: _C.envmap_rows(d, env, None), a.steps),
                 "backward, both gradients (k_rows_fill + k_envmap_rows_backward)": device_ms(lambda: _C.envmap_rows_backward(d, env, None, up, True, True), a.steps),
                 "backward, dL_dd alone": device_ms(lambda: _C.envmap_rows_backward(d, env, None, up, True, False), a.steps),
                 "backward, dL_denvmap alone (k_rows_fill + kernel)": device_ms(lambda: _C.envmap_rows_backward(d, env, None, up, False, True), a.steps)}
            r["forward_bytes"] = N * (12 + 4 * C)                # d, y (the map's texels come from the caches: at most He We C 4 bytes from memory)
            r["backward_bytes"] = N * (12 + 4 * C + 12) + 2 * He * We * C * 4   # d, grad_out, dL_dd; the fill and the atomics' floor
            r["forward_TB_per_s"] = round(r["forward_bytes"] / (r["k_envmap_rows"] * 1e-3) / 1e12, 3)
            r["backward_TB_per_s"] = round(r["backward_bytes"] / (r["backward, both gradients (k_rows_fill + k_envmap_rows_backward)"] * 1e-3) / 1e12, 3)
            s = stats_of(lambda: _C.envmap_rows_backward(d, env, None, up, False, True))
            if s is not None:
                r["dL_denvmap"] = s
            per[k] = r
            del up
        res["maps"][f"{He}x{We}"] = per
    # the yardstick: row kernels of the same form, on the packed rows of the same run
    g16 = th.randn(hit.shape[0], 16, generator=gen, device=dev)
    N = int(hit.shape[0])
    sh_f, sh_b = device_ms(lambda: _C.sh_rows(hit, 4, origin, view, None), a.steps), device_ms(lambda: _C.sh_rows_backward(hit, 4, origin, view, None, g16, True, True), a.steps)
    res["k_sh_rows"] = {"ms": sh_f, "TB_per_s": round(N * (12 + 4 + 64) / (sh_f * 1e-3) / 1e12, 3)}
    res["k_sh_rows_backward (+ fill)"] = {"ms": sh_b, "TB_per_s": round(N * (12 + 4 + 64 + 12) / (sh_b * 1e-3) / 1e12, 3)}
    del g16
    # the forward per C on the packed rows, 256 x 512: with DMR_ABLATE 67108864 on the ablation build, the other store shape
    res["forward_per_C"] = {}
    d = sets["packed"]
    for C in (1, 3, 4, 5, 8, 16):
        env = th.randn(MAPS[0][0], MAPS[0][1], C, generator=gen, device=dev)
        ms = device_ms(lambda: _C.envmap_rows(d, env, None), a.steps)
        res["forward_per_C"][str(C)] = {"ms": ms, "TB_per_s": round(int(d.shape[0]) * (12 + 4 * C) / (ms * 1e-3) / 1e12, 3)}
    print(json.dumps(res)); sys.exit(0)
# --compare
d0 = sets["background"]
N = int(d0.shape[0])
env = FG.EnvMap(*MAPS[0]).to(dev)
with th.no_grad():
    env.envmap.normal_()
g_y = th.randn(N, 3, generator=gen, device=dev)


def fused(d, up):
    y = env(d)
    return (y,) + th.autograd.grad(y, [d, env.envmap], grad_outputs=up)


def model(d, up):
    y = FG.envmap_rows(d, env.envmap)
    return (y,) + th.autograd.grad(y, [d, env.envmap], grad_outputs=up)


leaf = lambda: d0.clone().requires_grad_(True)
res["runs"] = []
for _ in range(3):
    r = {}
    r["torch_ms"], r["torch_peak_MiB"], gt = timed(model, a.torch_steps, (leaf(), g_y))
    r["fused_ms"], r["fused_peak_MiB"], gf = timed(fused, a.steps, (leaf(), g_y))
    r["time_ratio"], r["memory_ratio"] = round(r["torch_ms"] / r["fused_ms"], 3), round(r["torch_peak_MiB"] / max(r["fused_peak_MiB"], 0.1), 3)
    res["runs"].append(r)
res["rel_err_fused_vs_torch"] = {n: float(scenes.rel_err(p.detach().double().cpu().numpy(), q.detach().double().cpu().numpy()))
                                 for n, p, q in zip(("y", "dL_dd", "dL_denvmap"), gf, gt) if n != "dL_dd"}   # (dL_dd jumps at cell lines: tests/test_envmap_gpu.py)
del gt, gf
# the float32 deviation of the lookup on large maps against float64 torch on the device: a property of the lat-long arithmetic
res["float32_vs_float64"] = {}
for He, We in ((512, 1024), (1024, 2048)):
    e = th.randn(He, We, 3, generator=gen, device=dev)
    sub = d0[:: max(1, N // 500000)].contiguous()
    y64 = FG.envmap_rows(sub.double(), e.double())
    mine, torch32 = _C.envmap_rows(sub, e, None), FG.envmap_rows(sub, e)
    top = float(y64.abs().max())
    res["float32_vs_float64"][f"{He}x{We}"] = {"rows": int(sub.shape[0]), "fused": float((mine.double() - y64).abs().max()) / top,
                                               "float32_torch": float((torch32.double() - y64).abs().max()) / top}
print(json.dumps(res))
