"""The tri renderer's fragment lists without a GPU: the header's constants, dmesh_renderer_amd/fragments.py on hand-built
tensors against a per-pixel float64 loop (and gradcheck), and the Python plumbing of return_fragments over a stand-in `_C`."""
import os
import re

import numpy as np
import pytest
import torch as th

import test_capi_cpu
from standins import _StandIn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dmesh_renderer_amd.h")


def test_header_constants():
    src = open(HEADER).read()
    assert re.search(r"^#define DMR_FLAG_TRI_FRAGMENTS 64$", src, re.M)
    assert re.search(r"\bDMR_BUF_TRI_FRAGMENTS = 8\b", src)
    assert re.search(r"^#define DMR_FRAGMENTS_K\(flags\) ", src, re.M) and re.search(r"^#define DMR_FRAGMENTS_FLAGS\(k\) ", src, re.M)
    assert re.search(r"^#define DMR_ABI_VERSION 4$", src, re.M)
    import capi_ctypes
    assert test_capi_cpu._declared_functions() == sorted(capi_ctypes.EXPORTS)  # the macros declare no function


def test_header_macros_round_trip(tmp_path):
    """K travels in bits 8-15 next to the flag (compiled from the header with the host compiler)."""
    import shutil
    import subprocess
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc
    prog = tmp_path / "m.c"
    prog.write_text('#include "dmesh_renderer_amd.h"\n#include <stdio.h>\nint main(void) { int f = DMR_FLAG_ALPHA | DMR_FRAGMENTS_FLAGS(32);\n'
                    'printf("%d %d %d %d\\n", f, DMR_FRAGMENTS_K(f), DMR_FRAGMENTS_K(DMR_FLAG_ASYNC), DMR_FRAGMENTS_FLAGS(1)); return 0; }\n')
    subprocess.check_call([cc, "-I", os.path.dirname(HEADER), str(prog), "-o", str(tmp_path / "m")])
    out = subprocess.run([str(tmp_path / "m")], capture_output=True, text=True, check=True).stdout.split()
    assert out == [str(32 | 64 | (32 << 8)), "32", "0", str(64 | 256)]


# ---- fragments.py on a hand-built 2x2 image, K = 3 ------------------------------------------------------------------------
def _hand_built(dtype=th.float64):
    """B = 1, 2x2, K = 3, F = 5, P = 6.  Pixel (0,0): empty.  (0,1): one face.  (1,0): three faces, the middle one of opacity
    1.  (1,1): two faces, count 4 > K pretended (truncated list)."""
    from dmesh_renderer_amd import Fragments
    face = th.full((1, 3, 2, 2), -1, dtype=th.int32)
    bary = th.zeros(1, 3, 2, 2, 2, dtype=th.float32)
    count = th.zeros(1, 2, 2, dtype=th.int32)
    g = th.Generator().manual_seed(1)

    def put(y, x, ids):
        for k, f in enumerate(ids):
            face[0, k, y, x] = f
            u = float(th.rand((), generator=g)) * 0.6
            bary[0, k, 0, y, x], bary[0, k, 1, y, x] = u, float(th.rand((), generator=g)) * (0.9 - u)
        count[0, y, x] = len(ids)
    put(0, 1, [2])
    put(1, 0, [4, 1, 0])
    put(1, 1, [3, 4, 2])
    count[0, 1, 1] = 4
    faces = th.tensor([[0, 1, 2], [1, 2, 3], [2, 3, 4], [3, 4, 5], [5, 0, 2]], dtype=th.int32)
    opacity = th.tensor([0.3, 1.0, 0.55, 0.2, 0.7], dtype=dtype)
    attrs = th.randn(6, 4, generator=g, dtype=dtype)
    scale = th.rand(1, 5, generator=g, dtype=dtype) + 0.5
    return Fragments(face, bary, count), faces, opacity, attrs, scale


def _loop_reference(frag, faces, opacity, attrs, scale):
    """Per pixel, per slot, in Python float64."""
    B, K, H, W = frag.pix_to_face.shape
    C, F = attrs.shape[1], opacity.shape[0]
    w = np.zeros((B, K, H, W)); interp = np.zeros((B, K, C, H, W)); comp = np.zeros((B, C, H, W)); T = np.ones((B, 1, H, W))
    vis = np.zeros((B, F))
    for b in range(B):
        for y in range(H):
            for x in range(W):
                t = 1.0
                for k in range(K):
                    f = int(frag.pix_to_face[b, k, y, x])
                    if f < 0:
                        continue
                    u, v = float(frag.bary[b, k, 0, y, x]), float(frag.bary[b, k, 1, y, x])
                    i0, i1, i2 = (int(i) for i in faces[f])
                    a = (1 - u - v) * attrs[i0].numpy() + u * attrs[i1].numpy() + v * attrs[i2].numpy()
                    o = float(opacity[f])
                    w[b, k, y, x] = o * t
                    interp[b, k, :, y, x] = a
                    comp[b, :, y, x] += o * t * float(scale[b, f]) * a
                    vis[b, f] += o * t
                    t *= 1 - o
                T[b, 0, y, x] = t
    return w, interp, comp, T, vis


def test_helpers_match_a_per_pixel_loop():
    from dmesh_renderer_amd import fragments as FG
    frag, faces, opacity, attrs, scale = _hand_built()
    w, interp, comp, T, vis = _loop_reference(frag, faces, opacity, attrs, scale)
    tol = dict(rtol=0, atol=1e-7)  # (the barycentrics are float32 values, exactly representable in both computations)
    gw = FG.blend_weights(frag, opacity)
    assert tuple(gw.shape) == (1, 3, 2, 2)
    np.testing.assert_allclose(gw.numpy(), w, **tol)
    assert (gw[0, :, 0, 0] == 0).all() and gw[0, 2, 1, 0] == 0, "empty slots and a face behind an opaque one weigh nothing"
    gi = FG.interpolate(frag, faces, attrs)
    assert tuple(gi.shape) == (1, 3, 4, 2, 2)
    np.testing.assert_allclose(gi.numpy(), interp, **tol)
    gc, gT = FG.composite(frag, faces, opacity, attrs, face_scale=scale)
    assert tuple(gc.shape) == (1, 4, 2, 2) and tuple(gT.shape) == (1, 1, 2, 2)
    np.testing.assert_allclose(gc.numpy(), comp, **tol)
    np.testing.assert_allclose(gT.numpy(), T, **tol)
    assert gT[0, 0, 0, 0] == 1 and gT[0, 0, 1, 0] == 0
    g1, _ = FG.composite(frag, faces, opacity, attrs)
    np.testing.assert_allclose(g1.numpy(), _loop_reference(frag, faces, opacity, attrs, th.ones_like(scale))[2], **tol)
    gv = FG.face_visibility(frag, opacity, 5)
    assert tuple(gv.shape) == (1, 5)
    np.testing.assert_allclose(gv.numpy(), vis, **tol)
    np.testing.assert_allclose(float(gv.sum()), 4 - float(gT.sum()), **tol)


def test_composite_gradcheck():
    from dmesh_renderer_amd import fragments as FG
    frag, faces, opacity, attrs, scale = _hand_built()
    opacity = opacity.clone()
    opacity[1] = 0.9  # (at exactly 1 the product's derivative is still well defined, but keep gradcheck's steps inside [0, 1])
    leaves = [t.clone().requires_grad_(True) for t in (opacity, attrs, scale)]
    assert th.autograd.gradcheck(lambda o, a, s: FG.composite(frag, faces, o, a, face_scale=s), leaves, eps=1e-6, atol=1e-6)
    assert th.autograd.gradcheck(lambda o: FG.face_visibility(frag, o, 5), [leaves[0]], eps=1e-6, atol=1e-6)


# ---- TriRenderer(return_fragments=K) over a stand-in `_C` --------------------------------------------------------------------
class _FragStandIn(_StandIn):
    """tests/standins.py's stand-in, whose render_tris takes no `fragments`: this one records the keywords and returns the
    three tensors when asked."""

    def __init__(self, *a):
        super().__init__(*a)
        self.fwd_kw = []

    def render_tris(self, *args, rows=(0, 0), **kw):
        self.fwd_kw.append(dict(kw))
        H, W = args[11], args[12]
        out = super().render_tris(*args, rows=rows)
        if kw.get("alpha"):
            out = out[:2] + (th.zeros(self.B, 2, H, W, dtype=args[1].dtype),) + out[3:]
        k = kw.get("fragments", 0)
        if k:
            out = out + (th.full((self.B, k, H, W), -1, dtype=th.int32), th.zeros(self.B, k, 2, H, W), th.zeros(self.B, H, W, dtype=th.int32))
        return out


def _module_inputs(B, P, F):
    g = th.Generator().manual_seed(0)
    eye = th.eye(4, dtype=th.float64).repeat(B, 1, 1)
    return (th.randn(P, 3, generator=g, dtype=th.float64).requires_grad_(True), th.randint(0, P, (F, 3), generator=g), th.rand(P, 3, generator=g, dtype=th.float64).requires_grad_(True),
            th.rand(F, generator=g, dtype=th.float64).requires_grad_(True), eye, eye.clone(), th.rand(B, P, generator=g, dtype=th.float64), th.rand(B, F, generator=g, dtype=th.float64))


def test_renderer_keyword_over_a_stand_in(monkeypatch):
    import dmesh_renderer_amd as dmr
    B, P, F, H, W = 2, 5, 4, 8, 12
    settings = dmr.TriRenderSettings(H, W, th.zeros(3))
    inputs = _module_inputs(B, P, F)

    # the default call passes nothing new -- tests/standins.py's render_tris accepts no `fragments` (nor `alpha`) keyword
    plain = _StandIn(B, P, F, H, W, ())
    monkeypatch.setattr(dmr, "_C", plain)
    out = dmr.TriRenderer(settings)(*inputs)
    assert len(out) == 2

    fake = _FragStandIn(B, P, F, H, W, ())
    monkeypatch.setattr(dmr, "_C", fake)
    out = dmr.TriRenderer(settings)(*inputs)
    assert len(out) == 2 and fake.fwd_kw == [{}]

    color, depth, frag = dmr.TriRenderer(settings, return_fragments=3)(*inputs)
    assert fake.fwd_kw[-1] == {"fragments": 3}
    assert isinstance(frag, dmr.Fragments) and frag._fields == ("pix_to_face", "bary", "count")
    assert tuple(frag.pix_to_face.shape) == (B, 3, H, W) and tuple(frag.bary.shape) == (B, 3, 2, H, W) and tuple(frag.count.shape) == (B, H, W)
    assert color.requires_grad and depth.requires_grad and not any(t.requires_grad for t in frag)
    (color.sum() + depth.sum()).backward()  # the backward takes no new argument
    assert fake.kw[-1] == {}

    color, depth, alpha, frag = dmr.TriRenderer(settings, return_alpha=True, return_fragments=5)(*inputs)
    assert fake.fwd_kw[-1] == {"alpha": True, "fragments": 5}
    assert tuple(depth.shape) == (B, 1, H, W) and tuple(alpha.shape) == (B, 1, H, W) and isinstance(frag, dmr.Fragments)
    assert tuple(frag.pix_to_face.shape) == (B, 5, H, W) and not any(t.requires_grad for t in frag)

    t = [x.detach() for x in inputs]
    out = dmr.render_tri(t[0], t[1].int(), t[2], t[3], t[4], t[5], t[6], t[7], settings, return_fragments=2)
    assert len(out) == 3 and isinstance(out[2], dmr.Fragments) and fake.fwd_kw[-1] == {"fragments": 2}
    out = dmr.render_tri(t[0], t[1].int(), t[2], t[3], t[4], t[5], t[6], t[7], settings)
    assert len(out) == 2 and fake.fwd_kw[-1] == {}


def test_binding_refuses_a_bad_k_before_touching_a_device():
    """fragments outside 0..32 is an error of the binding itself (the library checks K of the flags again for C callers)."""
    from dmesh_renderer_amd import _C, scenes
    args = scenes.c_args(scenes.layered_sheets(1, 3, 1, 32, 32))
    for k in (33, -1):
        with pytest.raises(RuntimeError, match=r"0\.\.32"):
            _C.render_tris(*args, 32, 32, fragments=k)


def test_library_refuses_a_bad_k_through_last_error():
    """The C ABI's own check (a C caller has no binding in front of it): DMR_FLAG_TRI_FRAGMENTS with K = 0 or K > 32 in bits
    8-15 makes dmr_tri_forward fail with a message through dmr_last_error, before anything is allocated or launched; every
    other call ignores the flag's bits (here: a tri backward with nothing to back-propagate succeeds)."""
    import ctypes as C
    import capi_ctypes as lib_
    lib = lib_.load()
    requested = []

    @lib_.ALLOC_FN
    def alloc(ctx, which, nbytes):
        requested.append(which)
        return None

    dummy = (C.c_float * 4)()
    rendered = C.c_int(-1)
    for k in (0, 33, 255):
        sc = lib_.Scene(B=1, P=3, F=1, T=0, W=16, H=16, flags=64 | (k << 8))
        rc = lib.dmr_tri_forward(C.byref(sc), C.addressof(dummy), C.addressof(dummy), alloc, None, None, C.byref(rendered))
        assert rc != 0 and not requested
        msg = lib_.last_error()
        assert "DMR_FLAG_TRI_FRAGMENTS" in msg and "1..32" in msg and str(k) in msg, msg
    # P == 0: nothing to render; the check comes first all the same, and a good K then returns 0 without a request
    sc = lib_.Scene(B=1, P=0, F=0, T=0, W=16, H=16, flags=64 | (33 << 8))
    assert lib.dmr_tri_forward(C.byref(sc), C.addressof(dummy), C.addressof(dummy), alloc, None, None, C.byref(rendered)) != 0
    sc.flags = 64 | (4 << 8)
    assert lib.dmr_tri_forward(C.byref(sc), C.addressof(dummy), C.addressof(dummy), alloc, None, None, C.byref(rendered)) == 0
    assert rendered.value == 0 and not requested
