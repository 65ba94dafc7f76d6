"""The fused row MLP (fragments.mlp_rows_fused / RowMLP, csrc/dmr_mlp.hip) in the packed deferred-shading chain of
scripts/time_packed.py -- pack_slots_fused -> interpolate_packed_fused -> MLP (C -> 64 -> 3, tanh) -> composite_values_packed_fused
on a scenes.CONFIGS scene's fragment lists (default C4, fragments=4) -- once with nn.Sequential and once with a RowMLP on the
same Parameters.
  default    steps of: render the lists, one forward + backward of the chain with nn.Sequential, one with RowMLP -- for a kernel
             trace, so that the two new kernels stand next to the kernels torch launches for the same MLP in the same run.
  --compare  untraced: three alternating runs of each chain (wall time, peak torch.cuda.max_memory_allocated above the inputs);
             the two new kernels' device time by events beside nn.Sequential's forward and backward on the same rows; the bytes
             the forward must move, 4 N (Cin + Cout), and the TB/s of that it reaches; the chains' outputs against each other;
             dL_dW of the fused MLP at the full N against float64 torch on the device."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import torch as th
import dmesh_renderer_amd as dmr
from dmesh_renderer_amd import Fragments, _C, scenes
from dmesh_renderer_amd import fragments as FG

ap = argparse.ArgumentParser(); ap.add_argument("--config", default="C4"); ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--fragments", type=int, default=4); ap.add_argument("--channels", type=int, default=3)
ap.add_argument("--compare", action="store_true")
a = ap.parse_args()
dev = th.device("cuda:0")
cfg = scenes.CONFIGS[a.config]
B, H, W, K, C = cfg.B, cfg.H, cfg.W, a.fragments, a.channels
t = {k: v.to(dev) for k, v in scenes.make(a.config).items()}
renderer = dmr.TriRenderer(dmr.TriRenderSettings(H, W, t["bg"]), return_fragments=K)
names = ("verts", "faces", "verts_color", "faces_opacity", "mv_mats", "proj_mats", "verts_depth", "faces_intense")
faces = t["faces"].to(th.int32)
F, P = int(faces.shape[0]), int(t["verts"].shape[0])
gen = th.Generator().manual_seed(3)
attrs = th.randn(P, C, generator=gen).to(dev).requires_grad_(True)
opacity = t["faces_opacity"].clone().requires_grad_(True)
scale = (th.rand(B, F, generator=gen) + 0.5).to(dev).requires_grad_(True)
HID = 64
th.manual_seed(5)
seq = th.nn.Sequential(th.nn.Linear(C, HID), th.nn.Tanh(), th.nn.Linear(HID, 3)).to(dev)
row_mlp = FG.RowMLP.from_sequential(seq)   # the same Parameters
g_3, g_T = th.randn(B, 3, H, W, generator=gen).to(dev), th.randn(B, 1, H, W, generator=gen).to(dev)


def lists():
    with th.no_grad():
        frag = renderer(*(t[k] for k in names))[-1]
    return frag.pix_to_face, frag.bary.detach().requires_grad_(True)


def chain(mlp, face, bary):
    frag = Fragments(face, bary, None)
    packed = FG.pack_slots_fused(frag, F)
    x = FG.interpolate_packed_fused(frag, packed, faces, attrs)                             # [N,C]
    image, T = FG.composite_values_packed_fused(frag, packed, opacity, mlp(x), scale)
    return (image, T) + th.autograd.grad((image * g_3).sum() + (T * g_T).sum(), [attrs, bary, opacity, scale] + list(seq.parameters()))


def timed(fn, steps, fl, warm=3):
    for _ in range(warm):
        fn(*fl)
    th.cuda.synchronize(); base = th.cuda.memory_allocated(); th.cuda.reset_peak_memory_stats(); t0 = time.perf_counter()
    for _ in range(steps):
        out = fn(*fl)
    th.cuda.synchronize(); dt = (time.perf_counter() - t0) / steps
    return round(dt * 1e3, 4), round((th.cuda.max_memory_allocated() - base) / 2**20, 1), out


def device_ms(call, steps):
    ev = [th.cuda.Event(enable_timing=True) for _ in range(2)]
    for i in range(3 + steps):
        if i == 3: ev[0].record()
        call()
    ev[1].record(); th.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / steps


face, bary = lists()
n_used = int(FG.pack_slots_fused(Fragments(face, None, None), F).n_used)
res = {"config": a.config, "fragments": K, "channels": C, "hidden": HID, "image": [H, W], "views": B, "slots": face.numel(), "n_used": n_used}
if not a.compare:
    for _ in range(3 + a.steps):
        fl = lists()
        chain(seq, *fl); chain(row_mlp, *fl)
    th.cuda.synchronize()
    print(json.dumps(res)); sys.exit(0)
fl = (face, bary)
res["runs"] = []
for _ in range(3):
    r = {}
    r["sequential_ms"], r["sequential_peak_MiB"], gs = timed(lambda f, b: chain(seq, f, b), a.steps, fl)
    r["row_mlp_ms"], r["row_mlp_peak_MiB"], gf = timed(lambda f, b: chain(row_mlp, f, b), a.steps, fl)
    r["time_ratio"], r["memory_ratio"] = round(r["sequential_ms"] / r["row_mlp_ms"], 3), round(r["sequential_peak_MiB"] / max(r["row_mlp_peak_MiB"], 0.1), 3)
    res["runs"].append(r)
res["fused_faster_in_every_run"] = all(r["row_mlp_ms"] < r["sequential_ms"] for r in res["runs"])
res["fused_holds_less_in_every_run"] = all(r["row_mlp_peak_MiB"] < r["sequential_peak_MiB"] for r in res["runs"])
out_names = ("image", "T", "dL_dvert_attrs", "dL_dbary", "dL_dfaces_opacity", "dL_dface_scale", "dL_dW0", "dL_db0", "dL_dW1", "dL_db1")
res["rel_err_row_mlp_vs_sequential"] = {n: float(scenes.rel_err(x.detach().double().cpu().numpy(), y.detach().double().cpu().numpy())) for n, x, y in zip(out_names, gf, gs)}
# the MLP alone on the chain's rows: the two new kernels by events (no autograd), nn.Sequential's forward and backward beside them
packed = FG.pack_slots_fused(Fragments(face, None, None), F)
x = _C.interpolate_packed(face, bary.detach(), packed.row, packed.n_used, faces, attrs.detach(), packed.rows)
N = x.shape[0]
g_y = th.randn(N, 3, generator=th.Generator(device=dev).manual_seed(1), device=dev)
ws, bs = [w.detach() for w in row_mlp.weights], [b.detach() for b in row_mlp.biases]
xg = x.clone().requires_grad_(True)


def seq_fwd_bwd():
    th.autograd.grad(seq(xg), [xg] + list(seq.parameters()), grad_outputs=g_y)


with th.no_grad():
    seq_fwd = device_ms(lambda: seq(x), a.steps)
res["mlp_alone_ms"] = {
    "k_mlp_rows": round(device_ms(lambda: _C.mlp_rows(x, ws, bs, 1, 0, None), a.steps), 4),
    "k_mlp_rows_backward + k_mlp_reduce (all gradients)": round(device_ms(lambda: _C.mlp_rows_backward(x, ws, bs, 1, 0, None, g_y, True, [True] * 2, [True] * 2), a.steps), 4),
    "k_mlp_rows_backward (dL_dx only)": round(device_ms(lambda: _C.mlp_rows_backward(x, ws, bs, 1, 0, None, g_y, True, [False] * 2, [False] * 2), a.steps), 4),
    "nn.Sequential forward (no autograd)": round(seq_fwd, 4),
    "nn.Sequential forward + backward": round(device_ms(seq_fwd_bwd, a.steps), 4),
}
res["rows"] = N
res["forward_bytes"] = 4 * N * (C + 3)
res["forward_TB_per_s"] = round(res["forward_bytes"] / (res["mlp_alone_ms"]["k_mlp_rows"] * 1e-3) / 1e12, 3)
res["hidden_activation_bytes_torch_keeps"] = 4 * N * HID
# the weight gradients at the full N against float64 torch on the device
seq64 = th.nn.Sequential(th.nn.Linear(C, HID), th.nn.Tanh(), th.nn.Linear(HID, 3)).to(dev).double()
seq64.load_state_dict({k: v.double() for k, v in seq.state_dict().items()})
x64 = x.double().requires_grad_(True)
ref = th.autograd.grad(seq64(x64), [x64] + list(seq64.parameters()), grad_outputs=g_y.double())
dx, gw, gb = _C.mlp_rows_backward(x, ws, bs, 1, 0, None, g_y, True, [True] * 2, [True] * 2)
mine = [dx, gw[0], gb[0], gw[1], gb[1]]
res["full_size_rel_err_vs_float64"] = {n: float(scenes.rel_err(m.double().cpu().numpy(), r.cpu().numpy()))
                                       for n, m, r in zip(("dL_dx", "dL_dW0", "dL_db0", "dL_dW1", "dL_db1"), mine, ref)}
print(json.dumps(res))
