"""The packed deferred-shading path (fragments.pack_slots_fused, interpolate_packed_fused, composite_values_packed_fused) on a
scenes.CONFIGS scene's fragment lists (default C4, fragments=4; a tet config renders the tet lists), against the dense fused path
(interpolate_fused, composite_values_fused) on the same lists.
  default    steps of: render the lists, one forward + backward of the dense chain, one of the packed chain -- for a kernel trace, so
             that every new kernel stands next to its dense counterpart in the same run; prints the fill fraction n_used / (B K H W).
  --fill     the fill fraction only.
  --forward-only  k_interpolate_packed alone, for the two store shapes of the ablation build.
  --compare  untraced: one forward + backward of a chain with a two-layer MLP (C -> 64 -> 3, tanh) between the ends, packed against
             dense -- the dense path with the two permute(...).contiguous() a linear layer needs -- wall time and peak
             torch.cuda.max_memory_allocated above the inputs; the pack launches alone; each new kernel's device time by events."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import torch as th
import dmesh_renderer_amd as dmr
from dmesh_renderer_amd import Fragments, _C, scenes
from dmesh_renderer_amd import fragments as FG

ap = argparse.ArgumentParser(); ap.add_argument("--config", default="C4"); ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--fragments", type=int, default=4); ap.add_argument("--channels", type=int, default=3)
ap.add_argument("--fill", action="store_true"); ap.add_argument("--compare", action="store_true")
ap.add_argument("--forward-only", action="store_true", help="k_interpolate_packed alone: device time and a digest of its output (the "
                "store shapes of profiles/packed/store_shapes.txt: the ablation build, DMR_ABLATE=32768 against 0)")
a = ap.parse_args()
dev = th.device("cuda:0")
cfg = scenes.CONFIGS[a.config]
B, H, W, K, C = cfg.B, cfg.H, cfg.W, a.fragments, a.channels
t = {k: v.to(dev) for k, v in scenes.make(a.config).items()}
tet = cfg.kind == "tet"
if tet:
    renderer = dmr.TetRenderer(dmr.TetRenderSettings(H, W, t["bg"], 0), return_fragments=K)
    names = ("verts", "faces", "verts_color", "faces_opacity", "mv_mats", "proj_mats", "verts_depth", "faces_intense", "tets", "face_tets", "tet_faces")
else:
    renderer = dmr.TriRenderer(dmr.TriRenderSettings(H, W, t["bg"]), return_fragments=K)
    names = ("verts", "faces", "verts_color", "faces_opacity", "mv_mats", "proj_mats", "verts_depth", "faces_intense")
faces = t["faces"].to(th.int32)
F, P = int(faces.shape[0]), int(t["verts"].shape[0])
gen = th.Generator().manual_seed(3)
attrs = th.randn(P, C, generator=gen).to(dev).requires_grad_(True)
opacity = t["faces_opacity"].clone().requires_grad_(True)
scale = (th.rand(B, F, generator=gen) + 0.5).to(dev).requires_grad_(True)
HID = 64
w1 = (th.randn(C, HID, generator=gen) / C ** 0.5).to(dev).requires_grad_(True)
w2 = (th.randn(HID, 3, generator=gen) / HID ** 0.5).to(dev).requires_grad_(True)
g_c, g_3 = th.randn(B, C, H, W, generator=gen).to(dev), th.randn(B, 3, H, W, generator=gen).to(dev)
g_T = th.randn(B, 1, H, W, generator=gen).to(dev)


def lists():
    with th.no_grad():
        frag = renderer(*(t[k] for k in names))[-1]
    return frag.pix_to_face, frag.bary.detach().requires_grad_(True)


def dense_chain(face, bary):   # (the trace's chain: a pointwise shader, as scripts/time_deferred.py's)
    a_k = FG.interpolate_fused(Fragments(face, bary, None), faces, attrs)
    image, T = FG.composite_values_fused(Fragments(face, None, None), opacity, th.tanh(a_k), scale)
    return (image, T) + th.autograd.grad((image * g_c).sum() + (T * g_T).sum(), [attrs, bary, opacity, scale])


def packed_chain(face, bary):
    frag = Fragments(face, bary, None)
    packed = FG.pack_slots_fused(frag, F)
    rows = FG.interpolate_packed_fused(frag, packed, faces, attrs)
    image, T = FG.composite_values_packed_fused(frag, packed, opacity, th.tanh(rows), scale)
    return (image, T) + th.autograd.grad((image * g_c).sum() + (T * g_T).sum(), [attrs, bary, opacity, scale])


MLP_LEAVES = lambda bary: [attrs, bary, opacity, scale, w1, w2]


def dense_mlp(face, bary):
    a_k = FG.interpolate_fused(Fragments(face, bary, None), faces, attrs)                   # [B,K,C,H,W]
    x = a_k.permute(0, 1, 3, 4, 2).contiguous()                                             # rows for the linear layers
    y = (th.tanh(x.reshape(-1, C) @ w1) @ w2).reshape(B, K, H, W, 3)
    image, T = FG.composite_values_fused(Fragments(face, None, None), opacity, y.permute(0, 1, 4, 2, 3).contiguous(), scale)
    return (image, T) + th.autograd.grad((image * g_3).sum() + (T * g_T).sum(), MLP_LEAVES(bary))


def packed_mlp(face, bary):
    frag = Fragments(face, bary, None)
    packed = FG.pack_slots_fused(frag, F)
    x = FG.interpolate_packed_fused(frag, packed, faces, attrs)                             # [N,C]
    image, T = FG.composite_values_packed_fused(frag, packed, opacity, th.tanh(x @ w1) @ w2, scale)
    return (image, T) + th.autograd.grad((image * g_3).sum() + (T * g_T).sum(), MLP_LEAVES(bary))


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
res = {"config": a.config, "kind": cfg.kind, "fragments": K, "channels": C, "image": [H, W], "views": B, "faces": F, "verts": P,
       "slots": face.numel(), "n_used": n_used, "fill_fraction": round(n_used / face.numel(), 4)}
if a.fill:
    print(json.dumps(res)); sys.exit(0)
if a.forward_only:
    import hashlib
    packed = FG.pack_slots_fused(Fragments(face, None, None), F)
    call = lambda: _C.interpolate_packed(face, bary.detach(), packed.row, packed.n_used, faces, attrs.detach(), packed.rows)
    res["library"], res["DMR_ABLATE"] = os.path.basename(_C.library_path()), os.environ.get("DMR_ABLATE", "")
    res["k_interpolate_packed_ms"] = [round(device_ms(call, a.steps), 4) for _ in range(3)]
    res["out_sha1"] = hashlib.sha1(call().cpu().numpy().tobytes()).hexdigest()
    print(json.dumps(res)); sys.exit(0)
if not a.compare:
    for _ in range(3 + a.steps):
        fl = lists()
        dense_chain(*fl); packed_chain(*fl)
    th.cuda.synchronize()
    print(json.dumps(res)); sys.exit(0)
fl = (face, bary)
res["packed_mlp_ms"], res["packed_mlp_peak_MiB"], gp = timed(packed_mlp, a.steps, fl)
res["dense_mlp_ms"], res["dense_mlp_peak_MiB"], gd = timed(dense_mlp, a.steps, fl)
res["time_ratio_dense_over_packed"] = round(res["dense_mlp_ms"] / res["packed_mlp_ms"], 3)
res["memory_ratio_dense_over_packed"] = round(res["dense_mlp_peak_MiB"] / max(res["packed_mlp_peak_MiB"], 0.1), 3)
out_names = ("image", "T", "dL_dvert_attrs", "dL_dbary", "dL_dfaces_opacity", "dL_dface_scale", "dL_dw1", "dL_dw2")
res["rel_err_packed_vs_dense"] = {n: float(scenes.rel_err(x.detach().double().cpu().numpy(), y.detach().double().cpu().numpy())) for n, x, y in zip(out_names, gp, gd)}
# each kernel alone, device time by events (no autograd)
bary_d, at, op, sc = bary.detach(), attrs.detach(), opacity.detach(), scale.detach()
packed = FG.pack_slots_fused(Fragments(face, None, None), F)
rows = _C.interpolate_packed(face, bary_d, packed.row, packed.n_used, faces, at, packed.rows)
g_rows = th.randn(rows.shape, generator=th.Generator(device=dev).manual_seed(1), device=dev)
values = _C.interpolate_fragments(face, bary_d, faces, at)
g_out = th.randn(values.shape, generator=th.Generator(device=dev).manual_seed(1), device=dev)
kern = {
    "pack (k_pack_count + k_pack_scan + k_pack_write)": lambda: _C.pack_slots(face, F, face.numel()),
    "k_interpolate_packed": lambda: _C.interpolate_packed(face, bary_d, packed.row, packed.n_used, faces, at, packed.rows),
    "k_interpolate_fragments": lambda: _C.interpolate_fragments(face, bary_d, faces, at),
    "k_composite_values_packed": lambda: _C.composite_values_packed(face, packed.row, op, rows, sc),
    "k_composite_values": lambda: _C.composite_values(face, op, values, sc),
    "k_interpolate_packed_backward": lambda: _C.interpolate_packed_backward(face, bary_d, packed.row, packed.n_used, faces, at, g_rows, (True, True)),
    "k_interpolate_fragments_backward": lambda: _C.interpolate_fragments_backward(face, bary_d, faces, at, g_out, (True, True)),
    "k_composite_values_packed_backward": lambda: _C.composite_values_packed_backward(face, packed.row, packed.n_used, op, rows, sc, g_c, g_T, (True, True, True)),
    "k_composite_values_backward": lambda: _C.composite_values_backward(face, op, values, sc, g_c, g_T, (True, True, True)),
}
res["kernels_ms"] = {n: round(device_ms(call, a.steps), 4) for n, call in kern.items()}
res["rows_bytes"], res["planes_bytes"] = 4 * packed.rows * C, 4 * B * K * C * H * W
print(json.dumps(res))
