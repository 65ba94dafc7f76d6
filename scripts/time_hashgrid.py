"""The fused hash-grid encoding (fragments.hashgrid_rows_fused / HashGrid, csrc/dmr_hashgrid.hip) in front of the fused row MLP, on
the hit points of a scenes.CONFIGS scene's fragment lists (default C4, fragments=4): pack_slots_fused -> interpolate_packed_fused
(verts) -> HashGrid(16 levels, 2 features, T = 2^19, R = 16 .. 16 * 1.38^15) -> RowMLP(32, 64, 3).
  default    steps of: render the lists, one forward + backward of HashGrid -> RowMLP, fused -- for a kernel trace, so that the new
             kernels stand next to k_mlp_rows and k_mlp_rows_backward of the same run.
  --kernels  untraced: the new kernels' device time by events (forward; backward for both gradients, for dL/dx alone, for
             dL/dtable alone) on the lists' row order and on the same rows shuffled, the added bytes per second of the dL/dtable
             scatter, and -- on the ablation build (DMR_LIBRARY), whose DMR_ABLATE bits 1048576 / 2097152 / 4194304 / 16777216 / 8388608 select the
             forward's (row block, level chunk) grid / its per-lane row stores / a backward without the LDS table / its direct atomics one lane per row / counters in the
             backward (they cost time: a run of their own) -- the share of dL/dtable contributions per level that left as direct
             atomics.
  --compare  untraced: three alternating runs of the fused pair of Modules against the torch models (hashgrid_rows -> mlp_rows) on
             the device (wall time, peak torch.cuda.max_memory_allocated above the inputs), the outputs against each other, and
             dL_dtable at the full N against float64 torch on the device."""
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
th.manual_seed(5)
lo, hi = t["verts"].min(0).values - 1e-3, t["verts"].max(0).values + 1e-3
grid = FG.HashGrid(n_levels=16, features=2, log2_table_size=19, base_resolution=16, per_level_scale=1.38, lo=lo.tolist(), hi=hi.tolist()).to(dev)
mlp = FG.RowMLP(grid.out_features, 64, 3, activation="relu", out_activation="sigmoid").to(dev)
spec, params = grid.spec, [grid.table] + list(mlp.parameters())


def hit_points():
    with th.no_grad():
        frag = renderer(*(t[k] for k in names))[-1]
        packed = FG.pack_slots_fused(Fragments(frag.pix_to_face, None, None), F)
        return _C.interpolate_packed(frag.pix_to_face, frag.bary, packed.row, packed.n_used, faces, t["verts"], packed.rows)


def fused(x, g_y):
    y = mlp(grid(x))
    return (y,) + th.autograd.grad(y, [x] + params, grad_outputs=g_y)


def model(x, g_y):
    u = (x - grid.lo) / (grid.hi - grid.lo)
    y = FG.mlp_rows(FG.hashgrid_rows(u, grid.table, spec), list(mlp.weights), list(mlp.biases), activation=mlp.activation, out_activation=mlp.out_activation)
    return (y,) + th.autograd.grad(y, [x] + params, grad_outputs=g_y)


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


x = hit_points()
N = int(x.shape[0])
res = {"config": a.config, "fragments": K, "rows": N, "levels": 16, "features": 2, "log2_table_size": 19, "resolutions": list(spec.resolutions),
       "table_MiB": round(spec.offsets[-1] * 2 * 4 / 2**20, 1), "library": _C.library_path(), "DMR_ABLATE": os.environ.get("DMR_ABLATE", "")}
if not (a.compare or a.kernels):
    for _ in range(3 + a.steps):
        xs = hit_points().requires_grad_(True)
        fused(xs, th.ones(N, 3, device=dev))
    th.cuda.synchronize()
    print(json.dumps(res)); sys.exit(0)
g_y = th.randn(N, 3, generator=th.Generator(device=dev).manual_seed(1), device=dev)
if a.kernels:
    u = ((x - grid.lo) / (grid.hi - grid.lo)).contiguous()
    table, rl, lt = grid.table.detach(), list(spec.resolutions), spec.log2_table_size
    g_enc = th.randn(N, grid.out_features, generator=th.Generator(device=dev).manual_seed(2), device=dev)
    lib = ctypes.CDLL(_C.library_path())
    stats = getattr(lib, "dmr_hashgrid_stats", None)   # the ablation build's counters
    res["orders"] = {}
    for order, rows in (("lists", u), ("shuffled", u[th.randperm(N, device=dev)].contiguous())):
        r = {"k_hashgrid_rows": device_ms(lambda: _C.hashgrid_rows(rows, table, rl, lt, None), a.steps),
             "backward, both gradients (zero + k_hashgrid_rows_backward)": device_ms(lambda: _C.hashgrid_rows_backward(rows, table, rl, lt, None, g_enc, True, True), a.steps),
             "backward, dL_dx alone": device_ms(lambda: _C.hashgrid_rows_backward(rows, table, rl, lt, None, g_enc, True, False), a.steps),
             "backward, dL_dtable alone (zero + kernel)": device_ms(lambda: _C.hashgrid_rows_backward(rows, table, rl, lt, None, g_enc, False, True), a.steps)}
        added = N * 16 * 8 * 2 * 4
        r["unmerged_added_bytes"] = added
        r["dL_dtable_added_TB_per_s"] = round(added / (r["backward, dL_dtable alone (zero + kernel)"] * 1e-3) / 1e12, 3)
        r["forward_gather_plus_store_bytes"] = N * (16 * 8 * 8 + 128 + 12)
        if stats is not None and int(os.environ.get("DMR_ABLATE", "0")) & 8388608:
            buf = (ctypes.c_ulonglong * 32)()
            th.cuda.synchronize(); stats(None, 1)
            _C.hashgrid_rows_backward(rows, table, rl, lt, None, g_enc, False, True); th.cuda.synchronize()
            stats(buf, 1)
            r["direct_atomic_share_per_level"] = [round(buf[2 * l + 1] / max(buf[2 * l], 1), 4) for l in range(16)]
            r["direct_atomic_share"] = round(sum(buf[2 * l + 1] for l in range(16)) / max(sum(buf[2 * l] for l in range(16)), 1), 4)
        res["orders"][order] = r
    print(json.dumps(res)); sys.exit(0)
res["runs"] = []
for _ in range(3):
    r = {}
    r["torch_ms"], r["torch_peak_MiB"], gt = timed(model, a.torch_steps, (x.clone().requires_grad_(True), g_y))
    r["fused_ms"], r["fused_peak_MiB"], gf = timed(fused, a.steps, (x.clone().requires_grad_(True), g_y))
    r["time_ratio"], r["memory_ratio"] = round(r["torch_ms"] / r["fused_ms"], 3), round(r["torch_peak_MiB"] / max(r["fused_peak_MiB"], 0.1), 3)
    res["runs"].append(r)
res["fused_faster_in_every_run"] = all(r["fused_ms"] < r["torch_ms"] for r in res["runs"])
res["fused_holds_less_in_every_run"] = all(r["fused_peak_MiB"] < r["torch_peak_MiB"] for r in res["runs"])
out_names = ("y", "dL_dx", "dL_dtable", "dL_dW0", "dL_dW1", "dL_db0", "dL_db1")
res["rel_err_fused_vs_torch"] = {n: float(scenes.rel_err(p.detach().double().cpu().numpy(), q.detach().double().cpu().numpy())) for n, p, q in zip(out_names, gf, gt)}
del gt, gf
# the encoding's gradients at the full N against float64 torch on the device (the table's values as initialised, upstream N(0,1))
u = ((x - grid.lo) / (grid.hi - grid.lo)).contiguous()
g_enc = th.randn(N, grid.out_features, generator=th.Generator(device=dev).manual_seed(2), device=dev)
t64 = grid.table.detach().double().requires_grad_(True)
ref_t, = th.autograd.grad(FG.hashgrid_rows(u.double(), t64, spec), [t64], grad_outputs=g_enc.double())
_, mine_t = _C.hashgrid_rows_backward(u, grid.table.detach(), list(spec.resolutions), spec.log2_table_size, None, g_enc, False, True)
res["full_size_dL_dtable_rel_err_vs_float64"] = float(scenes.rel_err(mine_t.double().cpu().numpy(), ref_t.cpu().numpy()))
res["full_size_dL_dtable_max_abs_ref"] = float(ref_t.abs().max())
print(json.dumps(res))
