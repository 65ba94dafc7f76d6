"""The tet renderer's fragment lists without a GPU: the float64 checker of tests/tet_fragments_ref.py against the CPU oracle
(lists built from the float64 model of tests/tet_grad_ref.py), the header's constants, and the Python plumbing of
return_fragments over a stand-in `_C`."""
import os
import re

import numpy as np
import pytest
import torch as th

import tet_fragments_ref as TF
from grad_cases import scene
from standins import _FakeC
from tet_grad_ref import TetGradRef

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "dmesh_renderer_amd.h")).read()


@pytest.mark.parametrize("case", ["small", "opaque"])
def test_the_checker_reproduces_the_oracle_on_the_model_s_lists(oracle, case):
    """The lists of the kept pixels (TetGradRef.faces_of[:, :steps], float64 (u, v)) through composite64: the oracle's colour
    and depth to FWD_TOL ("opaque": faces of opacity 1, behind which the renderer goes on with T_EPS / 10)."""
    d, B, H, W, seed = scene(case)
    sc = oracle.scene_from_module_inputs(d, H, W, seed=seed)
    ocolor, odepth, oactive, ost = oracle.tet_forward(sc)
    ref = TetGradRef(d, H, W, ost)
    assert ref.kept_fraction >= 0.8, ref.kept_fraction
    face, bary, count = TF.model_lists(ref, d["verts"], d["faces"])
    assert face.shape[1] == int(count.max()) and (count > 0).sum() == ref.pix.numel()
    if case == "opaque":
        o = sc.faces_opacity[np.where(face >= 0, face, 0)]
        assert ((face >= 0) & (o >= 1.0)).any(), "the case must march through faces of opacity 1"
    color, depth, T = TF.composite64(sc, face, bary)
    keep = ref.keep.reshape(B, H, W).numpy()
    ec = float(np.abs(color - ocolor).transpose(0, 2, 3, 1)[keep].max())
    ed = float(np.abs(depth - odepth.reshape(B, 1, H, W))[:, 0][keep].max())
    et = float(np.abs(T - np.exp(ost.get("final_T").astype(np.float64).reshape(B, H, W)))[keep].max())
    print(f"\n{case}: {int(keep.sum())} kept pixels, composite64 vs oracle: colour {ec:.2e} depth {ed:.2e} final T {et:.2e}")
    assert ec <= TF.FWD_TOL and ed <= TF.FWD_TOL and et <= TF.FWD_TOL
    # a pixel without fragments: the bare background, depth 1, T 1
    assert (T[~keep] == 1).all() and (depth[:, 0][~keep] == 1).all()
    assert np.array_equal(color.transpose(0, 2, 3, 1)[~keep], np.broadcast_to(sc.bg.astype(np.float64)[:3], (int((~keep).sum()), 3)))
    # ... and the lists start and end where the oracle's march did
    last = np.take_along_axis(face, np.maximum(count - 1, 0)[:, None].astype(np.int64), axis=1)[:, 0]
    assert np.array_equal(face[:, 0][keep], ost.get("first_face").reshape(B, H, W)[keep])
    assert np.array_equal(last[keep], ost.get("last_face").reshape(B, H, W)[keep])


def test_header_constants():
    m = re.search(r"^#define DMR_FLAG_TET_FRAGMENTS \(1 << (\d+)\)$", HEADER, re.M)
    assert m and int(m.group(1)) == 16
    flag = 1 << int(m.group(1))
    assert flag & 0xff00 == 0, "bits 8-15 carry K"
    others = {n: int(v) for n, v in re.findall(r"^#define (DMR_FLAG_[A-Z_]+) (\d+)$", HEADER, re.M)}
    assert len(others) >= 8 and "DMR_FLAG_TRI_FRAGMENTS" in others
    assert all(v != flag and v & flag == 0 for v in others.values()), others
    assert re.search(r"\bDMR_BUF_TET_FRAGMENTS = 11\b", HEADER)
    assert re.search(r"^#define DMR_ABI_VERSION 4$", HEADER, re.M)
    assert re.search(r"^#define DMR_FRAGMENTS_K\(flags\) \(\(\(flags\) >> 8\) & 255\)$", HEADER, re.M)
    import capi_ctypes
    import test_capi_cpu
    assert test_capi_cpu._declared_functions() == sorted(capi_ctypes.EXPORTS)  # the macros declare no function


def test_library_refuses_a_bad_k_and_ignores_the_tri_flag():
    """The C ABI's own check: DMR_FLAG_TET_FRAGMENTS with K = 0 or K > 32 makes dmr_tet_forward fail before anything is
    allocated; a frame whose K steps alone exceed the 16 GiB budget fails the same way, naming K and the budget; P == 0
    requests no fragment buffer; the tri flag (64) is ignored by the tet call, K bits and all."""
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
    call = lambda sc: lib.dmr_tet_forward(C.byref(sc), C.addressof(dummy), C.addressof(dummy), C.addressof(dummy), alloc, None, None, C.byref(rendered))
    topo = dict(tets=C.addressof(dummy), face_tets=C.addressof(dummy), tet_faces=C.addressof(dummy))
    for k in (0, 33, 255):
        assert call(lib_.Scene(B=1, P=3, F=1, T=1, W=16, H=16, flags=(1 << 16) | (k << 8), **topo)) != 0 and not requested
        msg = lib_.last_error()
        assert "DMR_FLAG_TET_FRAGMENTS" in msg and "1..32" in msg and str(k) in msg, msg
    # 16 GiB / (32 steps * 4 bytes) = 134 217 728 tile pixels: one more tile row of a 16 384-wide frame is too many
    assert call(lib_.Scene(B=1, P=3, F=1, T=1, W=16384, H=8192 + 16, flags=(1 << 16) | (32 << 8), **topo)) != 0 and not requested
    msg = lib_.last_error()
    assert "K = 32" in msg and "16 GiB" in msg, msg
    # the tri flag with a bad K: not this call's business (it goes on to its scratch allocation, which this alloc refuses)
    assert call(lib_.Scene(B=1, P=3, F=1, T=1, W=16, H=16, flags=64 | (99 << 8), **topo)) != 0
    assert requested and 11 not in requested and "K" not in lib_.last_error(), lib_.last_error()
    del requested[:]
    # P == 0: the check comes first all the same; a good K then asks for no fragment buffer
    assert call(lib_.Scene(B=1, P=0, F=0, T=0, W=16, H=16, flags=(1 << 16) | (33 << 8))) != 0 and not requested
    call(lib_.Scene(B=1, P=0, F=0, T=0, W=16, H=16, flags=(1 << 16) | (4 << 8)))
    assert 11 not in requested


# ---- TetRenderer(return_fragments=K) over a stand-in `_C` -------------------------------------------------------------------
class _FragFakeC(_FakeC):
    """tests/standins.py's stand-in, whose render_tets takes no keyword but rows: this one records the keywords and returns
    the three tensors (and the two-channel depth) when asked."""

    def __init__(self):
        super().__init__()
        self.fwd_kw = []

    def render_tets(self, *args, rows=(0, 0), **kw):
        self.fwd_kw.append(dict(kw))
        out = super().render_tets(*args, rows=rows)
        B, (H, W) = args[5].shape[0], args[14:16]
        if kw.get("alpha"):
            out = out[:1] + (th.zeros(B, 2, H, W),) + out[2:]
        k = kw.get("fragments", 0)
        if k:
            out = out + (th.full((B, k, H, W), -1, dtype=th.int32), th.zeros(B, k, 2, H, W), th.zeros(B, H, W, dtype=th.int32))
        return out


def _module_inputs(B, P, F, T):
    g = th.Generator().manual_seed(0)
    eye = th.eye(4).repeat(B, 1, 1)
    return (th.randn(P, 3, generator=g), th.randint(0, P, (F, 3), generator=g), th.rand(P, 3, generator=g).requires_grad_(True),
            th.rand(F, generator=g).requires_grad_(True), eye, eye.clone(), th.rand(B, P, generator=g), th.rand(B, F, generator=g),
            th.randint(0, P, (T, 4), generator=g), th.randint(0, T, (F, 2), generator=g), th.randint(0, F, (T, 4), generator=g))


def test_renderer_keyword_over_a_stand_in(monkeypatch):
    import dmesh_renderer_amd as dmr
    B, P, F, T, H, W = 2, 5, 4, 3, 8, 12
    settings = dmr.TetRenderSettings(H, W, th.zeros(3), 0)
    inputs = _module_inputs(B, P, F, T)

    # the default call passes nothing new: tests/standins.py's render_tets accepts no `fragments` (nor `alpha`) keyword ...
    monkeypatch.setattr(dmr, "_C", _FakeC())
    assert len(dmr.TetRenderer(settings)(*inputs)) == 3
    # ... and _TetFn.apply gets the thirteen arguments it always got
    seen = []
    apply = dmr._TetFn.apply
    with monkeypatch.context() as mp:
        mp.setattr(dmr._TetFn, "apply", staticmethod(lambda *a: (seen.append(len(a)), apply(*a))[1]))
        dmr.TetRenderer(settings)(*inputs)
    assert seen == [13]

    fake = _FragFakeC()
    monkeypatch.setattr(dmr, "_C", fake)
    out = dmr.TetRenderer(settings)(*inputs)
    assert len(out) == 3 and fake.fwd_kw == [{}]

    color, depth, active, frag = dmr.TetRenderer(settings, return_fragments=3)(*inputs)
    assert fake.fwd_kw[-1] == {"fragments": 3}
    assert isinstance(frag, dmr.Fragments) and frag._fields == ("pix_to_face", "bary", "count")
    assert tuple(frag.pix_to_face.shape) == (B, 3, H, W) and tuple(frag.bary.shape) == (B, 3, 2, H, W) and tuple(frag.count.shape) == (B, H, W)
    assert active.dtype == th.bool and color.requires_grad and depth.requires_grad and not any(t.requires_grad for t in frag)
    (color.sum() + depth.sum()).backward()  # the backward takes no new argument
    assert fake.calls[-1][1] == {"rows": (0, 0)}

    out = dmr.TetRenderer(settings, return_alpha=True, return_fragments=5)(*inputs)
    assert fake.fwd_kw[-1] == {"alpha": True, "fragments": 5} and len(out) == 5
    color, depth, active, alpha, frag = out
    assert tuple(depth.shape) == (B, 1, H, W) and tuple(alpha.shape) == (B, 1, H, W) and active.dtype == th.bool
    assert isinstance(out[-1], dmr.Fragments) and tuple(frag.pix_to_face.shape) == (B, 5, H, W) and not any(t.requires_grad for t in frag)

    t = [x.detach() for x in inputs]
    ints = lambda *xs: [x.int() for x in xs]
    call = lambda **kw: dmr.render_tet(t[0], t[1].int(), *t[2:8], *ints(*t[8:11]), settings, **kw)
    out = call(return_fragments=2)
    assert len(out) == 4 and isinstance(out[-1], dmr.Fragments) and fake.fwd_kw[-1] == {"fragments": 2}
    out = call(return_alpha=True, return_fragments=2)
    assert len(out) == 5 and isinstance(out[-1], dmr.Fragments) and tuple(out[3].shape) == (B, 1, H, W)
    out = call()
    assert len(out) == 3 and fake.fwd_kw[-1] == {}
    with pytest.raises(TypeError):
        dmr.TetRenderer(settings, return_fragments=2, fragment_grads=True)  # no such keyword on the tet side


def test_sharded_module_refuses_the_option():
    import dmesh_renderer_amd as dmr
    from dmesh_renderer_amd.sharding import ShardedTetRenderer, _Shard
    settings = dmr.TetRenderSettings(32, 32, th.zeros(3), 0)
    with pytest.raises(ValueError, match="sharded"):
        ShardedTetRenderer(settings, impl=object(), return_fragments=4)
    # ... and so does the Function, whoever hands it a shard
    inputs = [x.detach() for x in _module_inputs(1, 5, 4, 3)]
    with pytest.raises(ValueError, match="sharded"):
        dmr._TetFn.apply(*inputs[:8], *(x.int() for x in inputs[8:]), settings, (0, 0), _Shard(_FragFakeC(), None, None), False, False, False, 4)


def test_binding_refuses_a_bad_k_before_touching_a_device():
    """fragments outside 0..32 is an error of the binding itself, the tri one's message."""
    from dmesh_renderer_amd import _C, scenes
    args = scenes.c_args(scenes.kuhn_tets(2, 1, 32, 32), tet=True)
    for k in (33, -1):
        with pytest.raises(RuntimeError, match=r"0\.\.32"):
            _C.render_tets(*args, 32, 32, 0, fragments=k)
