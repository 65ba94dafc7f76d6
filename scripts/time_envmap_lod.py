"""The fused pyramid lookup (fragments.envmap_pyramid_fused / envmap_lod_rows_fused / EnvMapPyramid, csrc/dmr_envmap_lod.hip) on a
scenes.CONFIGS scene (default C4, fragments=4, C = 3), on scripts/time_envmap.py's row sets: the BACKGROUND's rows (pixel_directions,
N = B H W) and the PACKED rows of the fragment lists (hit - camera origin), each also randomly permuted ("shuffled").  lod is
uniform over [0, L-1], one value per row; the pyramids are 256 x 512 and 1024 x 2048 with the full L (9 and 11).
  default    steps of: one forward + backward of EnvMapPyramid(256, 512) and of EnvMap(256, 512) on both row sets -- for a kernel
             trace, so that the new kernels stand next to k_envmap_rows and k_envmap_rows_backward of the same run.
  --kernels  untraced: the new kernels' device time by events on the four row sets (forward; backward for all three gradients, for
             each alone), next to the single-level pair on the same rows; the builder's forward and backward next to the torch
             builder on the device.
  --stats    on the ablation build (DMR_LIBRARY) with DMR_ABLATE bit 268435456: the share of dL/dpyramid contributions (a row's texel x
             chunk of nonzero weight) that leave as direct atomics, per pyramid size and row set, from the build's counters.
  --compare  untraced: three alternating runs of EnvMapPyramid against the torch models on the device (wall time, peak
             torch.cuda.max_memory_allocated above the inputs), and the deviation of y and the three gradients at that N from
             float64 torch on the device."""
import argparse, ctypes, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import torch as th
import dmesh_renderer_amd as dmr
from dmesh_renderer_amd import Fragments, _C, scenes
from dmesh_renderer_amd import fragments as FG

ap = argparse.ArgumentParser(); ap.add_argument("--config", default="C4"); ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--fragments", type=int, default=4); ap.add_argument("--torch-steps", type=int, default=2)
ap.add_argument("--compare", action="store_true"); ap.add_argument("--kernels", action="store_true"); ap.add_argument("--stats", action="store_true")
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
C = 3


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
    return sets


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


sets = row_sets()
res = {"config": a.config, "fragments": K, "rows": {k: int(v.shape[0]) for k, v in sets.items()}, "library": _C.library_path()}
gen = th.Generator(device=dev).manual_seed(2)
if a.stats:
    lib = ctypes.CDLL(_C.library_path())
    fn = getattr(lib, "dmr_envmap_lod_stats", None)
    if fn is None or not int(os.environ.get("DMR_ABLATE", "0") or 0) & (1 << 28):
        sys.exit("--stats needs the ablation build (DMR_LIBRARY) and DMR_ABLATE=268435456")
    res["DMR_ABLATE"], res["maps"] = int(os.environ["DMR_ABLATE"]), {}
    for He, We in MAPS:
        L = FG.EnvMapPyramid(He, We, 1).levels
        pyr = _C.envmap_pyramid(th.randn(He, We, C, generator=gen, device=dev), L)
        per = {"levels": L}
        for k, d in sets.items():
            N = int(d.shape[0])
            up, lod = th.randn(N, C, generator=gen, device=dev), th.rand(N, generator=gen, device=dev) * (L - 1)
            out = (ctypes.c_ulonglong * 2)()
            th.cuda.synchronize(); fn(None, 1)
            _C.envmap_lod_rows_backward(d, lod, pyr, He, We, L, None, up, False, False, True)
            th.cuda.synchronize(); fn(out, 1)
            per[k] = {"contributions": int(out[0]), "direct_atomics": int(out[1]), "share": round(out[1] / max(out[0], 1), 6)}
            del up, lod
        res["maps"][f"{He}x{We}"] = per
    print(json.dumps(res)); sys.exit(0)
if not (a.compare or a.kernels):
    pyr, env = FG.EnvMapPyramid(*MAPS[0]).to(dev), FG.EnvMap(*MAPS[0]).to(dev)
    lods = {k: th.rand(sets[k].shape[0], generator=gen, device=dev) * (pyr.levels - 1) for k in ("background", "packed")}
    for _ in range(3 + a.steps):
        for k in ("background", "packed"):
            d, lod = sets[k].clone().requires_grad_(True), lods[k].clone().requires_grad_(True)
            pyr(d, lod).sum().backward()
            d = sets[k].clone().requires_grad_(True)
            env(d).sum().backward()
    th.cuda.synchronize()
    print(json.dumps(res)); sys.exit(0)
if a.kernels:
    res["maps"] = {}
    for He, We in MAPS:
        L = FG.EnvMapPyramid(He, We, 1).levels
        env = th.randn(He, We, C, generator=gen, device=dev)
        pyr = _C.envmap_pyramid(env, L)
        per = {"levels": L, "T": int(pyr.shape[0])}
        for k, d in sets.items():
            N = int(d.shape[0])
            up, lod = th.randn(N, C, generator=gen, device=dev), th.rand(N, generator=gen, device=dev) * (L - 1)
            bwd = lambda nd, nl, npy: device_ms(lambda: _C.envmap_lod_rows_backward(d, lod, pyr, He, We, L, None, up, nd, nl, npy), a.steps)
            r = {"k_envmap_lod_rows": device_ms(lambda: _C.envmap_lod_rows(d, lod, pyr, He, We, L, None), a.steps),
                 "backward, all three gradients (k_rows_fill + k_envmap_lod_rows_backward)": bwd(True, True, True),
                 "backward, dL_dd alone": bwd(True, False, False), "backward, dL_dlod alone": bwd(False, True, False),
                 "backward, dL_dpyramid alone (k_rows_fill + kernel)": bwd(False, False, True),
                 "k_envmap_rows": device_ms(lambda: _C.envmap_rows(d, env, None), a.steps),
                 "k_envmap_rows_backward, both gradients (+ k_rows_fill)": device_ms(lambda: _C.envmap_rows_backward(d, env, None, up, True, True), a.steps)}
            r["forward_ratio"] = round(r["k_envmap_lod_rows"] / r["k_envmap_rows"], 3)
            r["backward_ratio"] = round(r["backward, all three gradients (k_rows_fill + k_envmap_lod_rows_backward)"] / r["k_envmap_rows_backward, both gradients (+ k_rows_fill)"], 3)
            r["forward_bytes"] = N * (12 + 4 + 4 * C)                # d, lod, y (the pyramid's texels come from the caches)
            r["forward_TB_per_s"] = round(r["forward_bytes"] / (r["k_envmap_lod_rows"] * 1e-3) / 1e12, 3)
            # one level pair for every row: the two levels' gathers without the spread over the pyramid
            one = th.full((N,), 0.5, device=dev)
            r["k_envmap_lod_rows, lod = 0.5 everywhere"] = device_ms(lambda: _C.envmap_lod_rows(d, one, pyr, He, We, L, None), a.steps)
            r["k_envmap_lod_rows, lod = 0 everywhere (one level read)"] = device_ms(lambda: _C.envmap_lod_rows(d, one * 0, pyr, He, We, L, None), a.steps)
            per[k] = r
            del up, lod, one
        # the builder next to the torch builder, forward and backward
        gp = th.randn(pyr.shape, generator=gen, device=dev)
        e = env.clone().requires_grad_(True)
        def torch_builder():
            th.autograd.grad(FG.envmap_pyramid(e, L), [e], grad_outputs=gp)
        per["builder"] = {"dmr_envmap_pyramid (L launches)": device_ms(lambda: _C.envmap_pyramid(env, L), a.steps),
                          "dmr_envmap_pyramid_backward (1 launch)": device_ms(lambda: _C.envmap_pyramid_backward(gp, He, We, L), a.steps),
                          "torch builder, forward": device_ms(lambda: FG.envmap_pyramid(env, L), a.steps),
                          "torch builder, forward + backward": device_ms(torch_builder, a.steps)}
        res["maps"][f"{He}x{We}"] = per
        del gp, e, pyr, env
    print(json.dumps(res)); sys.exit(0)
# --compare
d0 = sets["background"]
N = int(d0.shape[0])
mod = FG.EnvMapPyramid(*MAPS[0]).to(dev)
with th.no_grad():
    mod.envmap.normal_()
spec = (MAPS[0][0], MAPS[0][1], mod.levels)
g_y = th.randn(N, C, generator=gen, device=dev)
lod0 = th.rand(N, generator=gen, device=dev) * (mod.levels - 1)


def fused(d, lod, up):
    y = mod(d, lod)
    return (y,) + th.autograd.grad(y, [d, lod, mod.envmap], grad_outputs=up)


def model(d, lod, up, dtype=th.float32):
    e = mod.envmap.to(dtype)
    y = FG.envmap_lod_rows(d, lod, FG.envmap_pyramid(e, mod.levels), spec)
    return (y,) + th.autograd.grad(y, [d, lod, mod.envmap], grad_outputs=up)


leaves = lambda dtype=th.float32: (d0.to(dtype).clone().requires_grad_(True), lod0.to(dtype).clone().requires_grad_(True))
res["levels"], res["runs"] = mod.levels, []
for _ in range(3):
    r = {}
    r["torch_ms"], r["torch_peak_MiB"], gt = timed(model, a.torch_steps, (*leaves(), g_y))
    r["fused_ms"], r["fused_peak_MiB"], gf = timed(fused, a.steps, (*leaves(), g_y))
    r["time_ratio"], r["memory_ratio"] = round(r["torch_ms"] / r["fused_ms"], 3), round(r["torch_peak_MiB"] / max(r["fused_peak_MiB"], 0.1), 3)
    res["runs"].append(r)
# accuracy at that N against float64 torch on the device: the largest error and the rows above 1e-4 (dL_dd jumps at cell lines: a row that
# float32 puts into another cell than float64 differs by the jump)
g64 = model(*leaves(th.float64), g_y.double(), th.float64)
res["against_float64_torch"] = {}
for n, p, q32, q64 in zip(("y", "dL_dd", "dL_dlod", "dL_denvmap"), gf, gt, g64):
    top = float(q64.abs().max())
    err, err32 = (p.double() - q64).abs() / top, (q32.double() - q64).abs() / top
    res["against_float64_torch"][n] = {"fused_max": float(err.max()), "float32_torch_max": float(err32.max()),
                                       "fused_rows_above_1e-4": int((err.reshape(err.shape[0], -1).amax(1) > 1e-4).sum()),
                                       "float32_torch_rows_above_1e-4": int((err32.reshape(err32.shape[0], -1).amax(1) > 1e-4).sum())}
print(json.dumps(res))
