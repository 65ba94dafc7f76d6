"""Per-stage timing of the tri renderer on a scenes.CONFIGS scene (default C4), with the backward's gradient option."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import torch as th
from dmesh_renderer_amd import _C, scenes

ap = argparse.ArgumentParser(); ap.add_argument("--config", default="C4"); ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--grads", choices=("default", "exact", "camera"), default="default",
                help="backward variant: the reference's, exact_grads=True, camera_grads=True")
ap.add_argument("--alpha", action="store_true", help="forward and backward with the alpha output (TriRenderer(return_alpha=True))")
ap.add_argument("--fragments", type=int, default=0, help="forward with K fragment slots per pixel (TriRenderer(return_fragments=K))")
ap.add_argument("--fragment-grads", action="store_true",
                help="backward with a gradient for the fragments' barycentrics (TriRenderer(fragment_grads=True)); needs --fragments")
a = ap.parse_args()
if a.fragment_grads and not a.fragments: ap.error("--fragment-grads needs --fragments K")
dev = th.device("cuda:0")
cfg = scenes.CONFIGS[a.config]
B, H, W = cfg.B, cfg.H, cfg.W
d = scenes.make(a.config)
args = scenes.c_args(d, dev)
gc, gd = scenes.upstream_grads(B, H, W); gc, gd = gc.to(dev), gd.to(dev)
kw = {"default": {}, "exact": {"exact_grads": True}, "camera": {"camera_grads": True}}[a.grads]
akw = {}
if a.alpha:  # the depth image and its gradient gain a channel
    akw = {"alpha": True}; kw = dict(kw, alpha=True)
    gd = th.cat([gd, th.randn(B, 1, H, W, generator=th.Generator().manual_seed(5)).to(dev)], dim=1)
if a.fragments:
    akw = dict(akw, fragments=a.fragments)
gb = th.randn(B, a.fragments, 2, H, W, generator=th.Generator().manual_seed(9)).to(dev) if a.fragment_grads else None
def step():
    o = _C.render_tris(*args, H, W, **akw)
    fkw = {"fragment_grads": (o[7], gb)} if a.fragment_grads else {}  # (every stored pair receives a gradient)
    return o, _C.render_tris_backward(*args, gc, gd, o[0], *o[3:7], **kw, **fkw)
for _ in range(3): step()
_C.profile_enable(0xFFFFFFFF); th.cuda.synchronize(); t0 = time.perf_counter()
for _ in range(a.steps): o, g = step()
th.cuda.synchronize(); dt = (time.perf_counter() - t0) / a.steps
_C.profile_enable(0)
ms, cnt = _C.profile_collect()
st = {_C.stage_name(i): round(ms[i] / cnt[i], 4) for i in range(_C.NUM_STAGES) if cnt[i]}
print(json.dumps({"config": a.config, "grads": a.grads, "alpha": a.alpha, "fragments": a.fragments, "fragment_grads": a.fragment_grads, "faces": int(d["faces"].shape[0]), "image": [H, W],
                  "ms_per_step": round(dt * 1e3, 4), "stages_ms": st}))
