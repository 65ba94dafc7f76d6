"""The fused view-direction encoding (fragments.sh_rows_fused / ViewSH / packed_row_views_fused, csrc/dmr_sh.hip) beside the fused
hash grid in front of the fused row MLP, on the hit points of a scenes.CONFIGS scene's fragment lists (default C4, fragments=4):
pack_slots_fused -> packed_row_views_fused, interpolate_packed_fused (verts) -> cat(HashGrid(16 x 2, T = 2^19), ViewSH(4)) ->
RowMLP(48, 64, 3).
  default    steps of: render the lists, one forward + backward of that chain, fused -- for a kernel trace, so that the new kernels
             stand next to k_hashgrid_rows and k_mlp_rows of the same run.
  --kernels  untraced: the new kernels' device time by events, per degree (forward; backward for both gradients, for dL/dx
             alone, for dL/dorigin alone) and the row-to-view map, with the bytes each moves by construction per second.  On the
             ablation build (DMR_LIBRARY) DMR_ABLATE bit 33554432 runs every degree's OTHER store / load shape: the two runs
             together are the store-shape table.
  --compare  untraced: three alternating runs of ViewSH(4) against sh_rows on the device, and of the whole chain with and
             without the direction input (wall time, peak torch.cuda.max_memory_allocated above the inputs), what the th.cat and
             the copies of its gradient slices cost, and dL_dorigin at the full N against float64 torch on the device."""
import argparse, json, os, sys, time
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
th.manual_seed(5)
lo, hi = t["verts"].min(0).values - 1e-3, t["verts"].max(0).values + 1e-3
grid = FG.HashGrid(n_levels=16, features=2, log2_table_size=19, base_resolution=16, per_level_scale=1.38, lo=lo.tolist(), hi=hi.tolist()).to(dev)
sh = FG.ViewSH(4)
mlp = FG.RowMLP(grid.out_features + sh.out_features, 64, 3, activation="relu", out_activation="sigmoid").to(dev)
mlp_plain = FG.RowMLP(grid.out_features, 64, 3, activation="relu", out_activation="sigmoid").to(dev)
origin = FG.camera_origins(t["mv_mats"]).contiguous()


def hit_points():
    """-> (hit [N,3], view int32 [N])"""
    with th.no_grad():
        frag = renderer(*(t[k] for k in names))[-1]
        lists = Fragments(frag.pix_to_face, None, None)
        packed = FG.pack_slots_fused(lists, F)
        return _C.interpolate_packed(frag.pix_to_face, frag.bary, packed.row, packed.n_used, faces, t["verts"], packed.rows), FG.packed_row_views_fused(lists, packed)


def chain(x, view, g_y, o):
    y = mlp(th.cat([grid(x), sh(x, o, view)], 1))
    return (y,) + th.autograd.grad(y, [x, o, grid.table] + list(mlp.parameters()), grad_outputs=g_y)


def chain_without(x, view, g_y, o):
    y = mlp_plain(grid(x))
    return (y,) + th.autograd.grad(y, [x, grid.table] + list(mlp_plain.parameters()), grad_outputs=g_y)


def sh_fused(x, view, g_enc, o):
    y = FG.sh_rows_fused(x, 4, origin=o, row_view=view)
    return (y,) + th.autograd.grad(y, [x, o], grad_outputs=g_enc)


def sh_model(x, view, g_enc, o):
    y = FG.sh_rows(x, 4, origin=o, row_view=view)
    return (y,) + th.autograd.grad(y, [x, o], grad_outputs=g_enc)


def timed(fn, steps, args, warm=1):
    for _ in range(warm):
        fn(*args)
    th.cuda.synchronize(); base = th.cuda.memory_allocated(); th.cuda.reset_peak_memory_stats(); t0 = time.perf_counter()
    for _ in range(steps):
        out = fn(*args)
    th.cuda.synchronize(); dt = (time.perf_counter() - t0) / steps
    return round(dt * 1e3, 3), round((th.cuda.max_memory_allocated() - base) / 2**20, 1), out


def device_ms(call, steps):
    ev = [th.cuda.Event(enable_timing=True) for _ in range(2)]
    for i in range(3 + steps):
        if i == 3: ev[0].record()
        call()
    ev[1].record(); th.cuda.synchronize()
    return round(ev[0].elapsed_time(ev[1]) / steps, 4)


x, view = hit_points()
N = int(x.shape[0])
res = {"config": a.config, "fragments": K, "rows": N, "views": B, "rows_per_view": th.bincount(view.clamp(min=0).long(), minlength=B).tolist(),
       "library": _C.library_path(), "DMR_ABLATE": os.environ.get("DMR_ABLATE", "")}
if not (a.compare or a.kernels):
    for _ in range(3 + a.steps):
        xs, vs = hit_points()
        chain(xs.requires_grad_(True), vs, th.ones(N, 3, device=dev), origin.clone().requires_grad_(True))
    th.cuda.synchronize()
    print(json.dumps(res)); sys.exit(0)
if a.kernels:
    with th.no_grad():
        frag = renderer(*(t[k] for k in names))[-1]
        packed = FG.pack_slots_fused(Fragments(frag.pix_to_face, None, None), F)
    res["k_sh_fill + k_sh_row_views"] = {"ms": device_ms(lambda: _C.packed_row_views(packed.row, packed.rows), a.steps), "bytes": 4 * B * K * H * W + 8 * N}
    res["degrees"] = {}
    for degree in (1, 2, 3, 4):
        C = degree * degree
        g_enc = th.randn(N, C, generator=th.Generator(device=dev).manual_seed(2), device=dev)
        r = {"k_sh_rows": device_ms(lambda: _C.sh_rows(x, degree, origin, view, None), a.steps),
             "backward, both gradients (k_sh_fill + k_sh_rows_backward)": device_ms(lambda: _C.sh_rows_backward(x, degree, origin, view, None, g_enc, True, True), a.steps),
             "backward, dL_dx alone": device_ms(lambda: _C.sh_rows_backward(x, degree, origin, view, None, g_enc, True, False), a.steps),
             "backward, dL_dorigin alone (k_sh_fill + kernel)": device_ms(lambda: _C.sh_rows_backward(x, degree, origin, view, None, g_enc, False, True), a.steps)}
        r["forward_bytes"] = N * (12 + 4 + 4 * C)            # x, row_view, y
        r["backward_bytes"] = N * (12 + 4 + 4 * C + 12)      # x, row_view, grad_out, dL_dx
        r["forward_TB_per_s"] = round(r["forward_bytes"] / (r["k_sh_rows"] * 1e-3) / 1e12, 3)
        r["backward_TB_per_s"] = round(r["backward_bytes"] / (r["backward, both gradients (k_sh_fill + k_sh_rows_backward)"] * 1e-3) / 1e12, 3)
        res["degrees"][str(degree)] = r
    print(json.dumps(res)); sys.exit(0)
g_y = th.randn(N, 3, generator=th.Generator(device=dev).manual_seed(1), device=dev)
g_enc = th.randn(N, 16, generator=th.Generator(device=dev).manual_seed(2), device=dev)
leaf = lambda: (x.clone().requires_grad_(True), view)
org = lambda: origin.clone().requires_grad_(True)
res["sh_runs"], res["chain_runs"] = [], []
for _ in range(3):
    r = {}
    r["torch_ms"], r["torch_peak_MiB"], gt = timed(sh_model, a.torch_steps, (*leaf(), g_enc, org()))
    r["fused_ms"], r["fused_peak_MiB"], gf = timed(sh_fused, a.steps, (*leaf(), g_enc, org()))
    r["time_ratio"], r["memory_ratio"] = round(r["torch_ms"] / r["fused_ms"], 3), round(r["torch_peak_MiB"] / max(r["fused_peak_MiB"], 0.1), 3)
    res["sh_runs"].append(r)
    c = {}
    c["without_direction_ms"], c["without_direction_peak_MiB"], _ = timed(chain_without, a.steps, (*leaf(), g_y, org()))
    c["with_direction_ms"], c["with_direction_peak_MiB"], _ = timed(chain, a.steps, (*leaf(), g_y, org()))
    res["chain_runs"].append(c)
res["sh_fused_faster_in_every_run"] = all(r["fused_ms"] < r["torch_ms"] for r in res["sh_runs"])
res["sh_fused_holds_less_in_every_run"] = all(r["fused_peak_MiB"] < r["torch_peak_MiB"] for r in res["sh_runs"])
res["rel_err_fused_vs_torch"] = {n: float(scenes.rel_err(p.detach().double().cpu().numpy(), q.detach().double().cpu().numpy()))
                                 for n, p, q in zip(("y", "dL_dx", "dL_dorigin"), gf, gt)}
del gt, gf
# what the th.cat of the two encodings and the contiguous copies of its gradient's two column slices cost, by events
enc_grid, enc_sh = th.randn(N, 32, device=dev), th.randn(N, 16, device=dev)
g48 = th.randn(N, 48, device=dev)
res["cat_ms"] = device_ms(lambda: th.cat([enc_grid, enc_sh], 1), a.steps)
res["cat_backward_slices_ms"] = device_ms(lambda: (g48[:, :32].contiguous(), g48[:, 32:].contiguous()), a.steps)
del enc_grid, enc_sh, g48
# dL_dorigin at the full N against float64 torch on the device
o64 = origin.double().requires_grad_(True)
ref_o, = th.autograd.grad(FG.sh_rows(x.double(), 4, origin=o64, row_view=view), [o64], grad_outputs=g_enc.double())
_, mine_o = _C.sh_rows_backward(x, 4, origin, view, None, g_enc, False, True)
res["full_size_dL_dorigin_rel_err_vs_float64"] = float((mine_o.double() - ref_o).abs().max() / ref_o.abs().max())
res["full_size_dL_dorigin_max_abs_ref"] = float(ref_o.abs().max())
print(json.dumps(res))
