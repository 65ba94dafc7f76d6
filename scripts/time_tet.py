"""Per-stage timing of the tet renderer on a Kuhn-lattice scene (default C3: m=16, 800x800)."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import numpy as np, torch as th
from dmesh_renderer_amd import _C, scenes

ap = argparse.ArgumentParser(); ap.add_argument("--m", type=int, default=16); ap.add_argument("--size", type=int, default=800)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--full-grads", action="store_true", help="backward with dL/dverts and dL/dfaces_intense (TetRenderer(full_grads=True))")
ap.add_argument("--camera-grads", action="store_true", help="backward with those and the matrices' (TetRenderer(camera_grads=True))")
ap.add_argument("--alpha", action="store_true", help="forward and backward with the alpha output (TetRenderer(return_alpha=True))")
ap.add_argument("--fragments", type=int, default=0, help="forward with K fragment slots per pixel (TetRenderer(return_fragments=K))")
ap.add_argument("--fragment-grads", action="store_true",
                help="backward with a gradient for the fragments' barycentrics (TetRenderer(fragment_grads=True)); needs --fragments")
a = ap.parse_args()
if a.fragment_grads and not a.fragments: ap.error("--fragment-grads needs --fragments K")
kw = {"camera_grads": True} if a.camera_grads else ({"full_grads": True} if a.full_grads else {})
dev = th.device("cuda:0"); H = W = a.size
d = scenes.kuhn_tets(a.m, 1, H, W)
args = scenes.c_args(d, dev, tet=True)
gc, gd = scenes.upstream_grads(1, H, W); gc, gd = gc.to(dev), gd.to(dev)
akw = {}
if a.alpha:  # the depth image and its gradient gain a channel
    akw = {"alpha": True}; kw = dict(kw, alpha=True)
    gd = th.cat([gd, th.randn(1, 1, H, W, generator=th.Generator().manual_seed(5)).to(dev)], dim=1)
if a.fragments:
    akw = dict(akw, fragments=a.fragments)
gb = th.randn(1, a.fragments, 2, H, W, generator=th.Generator().manual_seed(9)).to(dev) if a.fragment_grads else None
def step():
    o = _C.render_tets(*args, H, W, 0, **akw)
    fkw = {"fragment_grads": (o[7], gb)} if a.fragment_grads else {}  # (every stored pair receives a gradient; implies full_grads)
    g = _C.render_tets_backward(*args, gc, gd, *o[3:7], **kw, **fkw)
    return o, g
for _ in range(3): step()
_C.profile_enable(0xFFFFFFFF); th.cuda.synchronize(); t0 = time.perf_counter()
for _ in range(a.steps): o, g = step()
th.cuda.synchronize(); dt = (time.perf_counter() - t0) / a.steps
_C.profile_enable(0)
ms, cnt = _C.profile_collect()
st = {_C.stage_name(i): round(ms[i] / cnt[i], 4) for i in range(_C.NUM_STAGES) if cnt[i]}
print(json.dumps({"alpha": a.alpha, "fragments": a.fragments, "fragment_grads": a.fragment_grads, "tets": int(d["tets"].shape[0]), "faces": int(d["faces"].shape[0]), "image": [H, W], "ms_per_step": round(dt * 1e3, 4),
                  "Mpix_s": round(H * W / dt / 1e6, 1), "active_frac": round(float(o[2].mean()), 3), "stages_ms": st}))
