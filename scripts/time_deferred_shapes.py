"""Device time of the four calls of the deferred-shading unit under the library DMR_LIBRARY names (default: the package's own):
20 calls captured into one HIP graph, the graph replayed, timed by events, the best of three replays (no launch gaps).  C4 lists
with fragments=4, C = 3 and C = 32; GB/s is 4 B K C H W over the time.  This is how profiles/deferred/lane_shapes.txt was taken:
one fresh process per build, the builds differing in the pixel-to-lane mapping of csrc/dmr_interp.hip alone -- copy csrc/, make
the edit that file lists for the variant, compile the copy with build.py's hipcc line into another libdmesh_renderer_hip.so, and

    DMR_LIBRARY=/path/to/variant/libdmesh_renderer_hip.so python scripts/time_deferred_shapes.py

(the binding of this tree loads any build of the same C ABI)."""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import torch as th
from dmesh_renderer_amd import _C, scenes
dev = th.device("cuda:0")
cfg = scenes.CONFIGS["C4"]
B, H, W, K = cfg.B, cfg.H, cfg.W, 4
d = scenes.make("C4")
args = scenes.c_args(d, dev)
faces = d["faces"].to(dev).to(th.int32)
F, P = int(faces.shape[0]), int(d["verts"].shape[0])
o = _C.render_tris(*args, H, W, fragments=K)
face, bary = o[7], o[8]
op = d["faces_opacity"].to(dev)
res = {"library": os.environ.get("DMR_LIBRARY", "default")}
N = 20
for C in (3, 32):
    gen = th.Generator().manual_seed(3)
    at = th.randn(P, C, generator=gen).to(dev)
    sc = (th.rand(B, F, generator=gen) + 0.5).to(dev)
    g_image = th.randn(B, C, H, W, generator=gen).to(dev); g_T = th.randn(B, 1, H, W, generator=gen).to(dev)
    values = _C.interpolate_fragments(face, bary, faces, at)
    g_out = th.randn(values.shape, device=dev)
    plane = 4 * B * K * C * H * W
    kern = {
        "interpolate_fragments": lambda: _C.interpolate_fragments(face, bary, faces, at),
        "composite_values": lambda: _C.composite_values(face, op, values, sc),
        "interpolate_fragments_backward": lambda: _C.interpolate_fragments_backward(face, bary, faces, at, g_out, (True, True)),
        "composite_values_backward": lambda: _C.composite_values_backward(face, op, values, sc, g_image, g_T, (True, True, True)),
        "composite_values_backward_dvalues_only": lambda: _C.composite_values_backward(face, op, values, sc, g_image, None, (False, True, False)),
        "composite_fragments": lambda: _C.composite_fragments(face, bary, faces, op, at, sc),
    }
    for n, call in kern.items():
        side = th.cuda.Stream(); side.wait_stream(th.cuda.current_stream())
        with th.cuda.stream(side):
            call(); call()
        th.cuda.current_stream().wait_stream(side); th.cuda.synchronize()
        g = th.cuda.CUDAGraph()
        with th.cuda.graph(g):
            keep = [call() for _ in range(N)]
        g.replay(); g.replay(); th.cuda.synchronize()
        best = 1e9
        for _ in range(3):
            ev = [th.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record(); g.replay(); ev[1].record(); th.cuda.synchronize()
            best = min(best, ev[0].elapsed_time(ev[1]) / N)
        res[f"C{C} {n}"] = {"us": round(best * 1e3, 2), "plane_GBps": round(plane / best / 1e6, 1)}
        del g, keep
print(json.dumps(res))
