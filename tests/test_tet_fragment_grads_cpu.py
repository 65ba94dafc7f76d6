"""The tet renderer's fragment_grads without a GPU: the header's flag and buffer ids, the library's own check of K, the Python
plumbing over a stand-in `_C`, and the float64 model's synthetic pair set (tests/tet_fragment_grads_ref.py) that
tests/test_tet_fragment_grads_gpu.py runs on the device."""
import os
import re

import numpy as np
import pytest
import torch as th

import tet_fragment_grads_ref as TFG
from grad_cases import MATS_TOL, TET_VERTS_TOL
from standins import _FakeC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "dmesh_renderer_amd.h")).read()
FLAG = 1 << 17


def _flags():
    """Every DMR_FLAG_* of the header, whether written as a decimal literal or as (1 << n)."""
    out = {n: int(v) for n, v in re.findall(r"^#define (DMR_FLAG_[A-Z_]+) (\d+)$", HEADER, re.M)}
    out.update({n: 1 << int(v) for n, v in re.findall(r"^#define (DMR_FLAG_[A-Z_]+) \(1 << (\d+)\)$", HEADER, re.M)})
    return out


def test_header_defines_the_flag_and_the_two_buffers():
    assert re.search(r"^#define DMR_FLAG_TET_FRAGMENT_GRADS \(1 << 17\)$", HEADER, re.M)
    flags = _flags()
    assert flags["DMR_FLAG_TET_FRAGMENT_GRADS"] == FLAG and flags["DMR_FLAG_TET_FRAGMENTS"] == 1 << 16 and len(flags) >= 10
    assert len(set(flags.values())) == len(flags) and all(v & (v - 1) == 0 for v in flags.values()), flags
    assert FLAG & 0xff00 == 0, "bits 8-15 carry K"
    assert re.search(r"\bDMR_BUF_TET_FRAGMENT_FACES = 12\b", HEADER) and re.search(r"\bDMR_BUF_TET_FRAGMENT_BARY_GRADS = 13\b", HEADER)
    assert re.search(r"^#define DMR_ABI_VERSION 4$", HEADER, re.M)
    m = re.search(r"^#define DMR_FRAGMENTS_K\(flags\) (.*)$", HEADER, re.M)
    k_of = lambda x: eval(m.group(1), {"flags": x})
    for k in (1, 2, 8, 32, 255):
        assert k_of(FLAG | (k << 8)) == k and k_of(FLAG | (1 << 16) | (k << 8) | 2 | 16 | 32) == k
        assert (FLAG | (k << 8)) & 255 == 0


def test_library_refuses_a_bad_k_before_any_request():
    """dmr_tet_backward with DMR_FLAG_TET_FRAGMENT_GRADS and K = 0 (or K > 32) fails with a message through dmr_last_error
    before it calls `alloc`, whatever the scene; without the flag the K bits are ignored (here: nothing to back-propagate, the
    call succeeds), and a good K with nothing to back-propagate requests neither input."""
    import ctypes as C
    import capi_ctypes as lib_
    lib = lib_.load()
    requested = []

    @lib_.ALLOC_FN
    def alloc(ctx, which, nbytes):
        requested.append(which)
        return None

    dummy = (C.c_float * 16)()
    p = C.addressof(dummy)

    def backward(flags, P=3, F=1, T=1):
        topo = dict(tets=p, face_tets=p, tet_faces=p) if P else {}
        sc = lib_.Scene(B=1, P=P, F=F, T=T, W=16, H=16, flags=flags, **topo)
        return lib.dmr_tet_backward(C.byref(sc), p, p, None, None, None, None, p, p, alloc, None, None)

    for k in (0, 33, 255):
        assert backward(FLAG | (k << 8)) != 0 and not requested
        msg = lib_.last_error()
        assert "DMR_FLAG_TET_FRAGMENT_GRADS" in msg and "1..32" in msg and str(k) in msg, msg
        assert backward(FLAG | 2 | 16 | (k << 8), P=0, F=0, T=0) != 0 and not requested  # the check comes first, whatever the scene
    assert backward(33 << 8, P=0, F=0, T=0) == 0 and backward((1 << 16) | (99 << 8), P=0, F=0, T=0) == 0 and not requested
    assert backward(FLAG | (4 << 8), P=0, F=0, T=0) == 0 and 12 not in requested and 13 not in requested


# ---- TetRenderer(return_fragments=K, fragment_grads=True) over a stand-in `_C` -----------------------------------------------
class _FragGradFakeC(_FakeC):
    """tests/standins.py's stand-in with the forward's `fragments` and `alpha` keywords (face ids 0, a bary that is a plain
    tensor, count 1), a backward that records its keywords but `rows`, and the attribute by which the binding says that its
    render_tets_backward takes fragment_grads."""
    SUPPORTS_TET_FRAGMENT_GRADS = True

    def __init__(self):
        super().__init__()
        self.kw = []

    def render_tets(self, *args, rows=(0, 0), **kw):
        out = super().render_tets(*args, rows=rows)
        B, (H, W) = args[5].shape[0], args[14:16]
        if kw.get("alpha"):
            out = out[:1] + (th.zeros(B, 2, H, W),) + out[2:]
        k = kw.get("fragments", 0)
        if k:
            out = out + (th.zeros(B, k, H, W, dtype=th.int32), th.full((B, k, 2, H, W), 0.25), th.ones(B, H, W, dtype=th.int32))
        return out

    def render_tets_backward(self, *args, rows=(0, 0), **kw):
        self.kw.append(kw)
        return super().render_tets_backward(*args, **kw)


def _module_inputs(B, P, F, T):
    g = th.Generator().manual_seed(0)
    eye = th.eye(4).repeat(B, 1, 1)
    return [th.randn(P, 3, generator=g).requires_grad_(True), th.randint(0, P, (F, 3), generator=g), th.rand(P, 3, generator=g).requires_grad_(True),
            th.rand(F, generator=g), eye, eye.clone(), th.rand(B, P, generator=g), th.rand(B, F, generator=g),
            th.randint(0, P, (T, 4), generator=g), th.randint(0, T, (F, 2), generator=g), th.randint(0, F, (T, 4), generator=g)]


def test_wrapper_routes_the_keyword_only_with_the_option(monkeypatch):
    import dmesh_renderer_amd as dmr
    B, P, F, T, H, W, K = 2, 5, 4, 3, 8, 12, 3
    settings = dmr.TetRenderSettings(H, W, th.zeros(3), 0)
    inputs = _module_inputs(B, P, F, T)
    fake = _FragGradFakeC()
    monkeypatch.setattr(dmr, "_C", fake)

    # without the option: constants, and a backward without any keyword
    color, depth, active, frag = dmr.TetRenderer(settings, return_fragments=K)(*inputs)
    assert not any(t.requires_grad for t in frag)
    (color.sum() + depth.sum()).backward()
    assert fake.kw[-1] == {}
    # ... and the default call's apply gets the thirteen arguments it always got
    seen = []
    apply = dmr._TetFn.apply
    with monkeypatch.context() as mp:
        mp.setattr(dmr._TetFn, "apply", staticmethod(lambda *a: (seen.append(len(a)), apply(*a))[1]))
        dmr.TetRenderer(settings)(*inputs)
    assert seen == [13]

    # with it: bary is differentiable, face and count are not; full_grads travels whenever the option is set, the keyword only
    # when a gradient for bary arrives
    r = dmr.TetRenderer(settings, return_fragments=K, fragment_grads=True)
    assert r.fragment_grads and not r.full_grads
    color, depth, active, frag = r(*inputs)
    assert frag.bary.requires_grad and not frag.pix_to_face.requires_grad and not frag.count.requires_grad and not active.requires_grad
    n = len(fake.kw)
    inputs[0].grad = None
    (color.sum() + depth.sum()).backward()
    assert len(fake.kw) == n + 1 and fake.kw[-1] == {"full_grads": True}
    assert inputs[0].grad is not None and bool((inputs[0].grad == 1.0).all())  # (the stand-in's verts piece: the images' gradient reaches verts)
    color, depth, active, frag = r(*inputs)
    up = th.arange(B * K * 2 * H * W, dtype=th.float32).reshape(B, K, 2, H, W)
    inputs[0].grad = None
    (frag.bary * up).sum().backward()
    assert set(fake.kw[-1]) == {"full_grads", "fragment_grads"} and fake.kw[-1]["full_grads"] is True
    face, g = fake.kw[-1]["fragment_grads"]
    assert face.dtype == th.int32 and tuple(face.shape) == (B, K, H, W) and th.equal(face, frag.pix_to_face)
    assert g.dtype == th.float32 and g.is_contiguous() and th.equal(g, up)
    assert inputs[0].grad is not None and tuple(inputs[0].grad.shape) == (P, 3)
    # with the other options the keyword joins theirs: camera_grads without a matrix that needs a gradient is level 1 ...
    color, depth, active, alpha, frag = dmr.TetRenderer(settings, camera_grads=True, return_alpha=True, return_fragments=K, fragment_grads=True)(*inputs)
    (color.sum() + (frag.bary * up).sum()).backward()
    assert set(fake.kw[-1]) == {"full_grads", "alpha", "fragment_grads"}
    # ... and with one, level 2
    mats = list(inputs)
    mats[4] = inputs[4].clone().requires_grad_(True)
    r2 = dmr.TetRenderer(settings, camera_grads=True, return_fragments=K, fragment_grads=True)
    color, depth, active, frag = r2(*mats)
    (color.sum() + (frag.bary * up).sum()).backward()
    assert set(fake.kw[-1]) == {"camera_grads", "fragment_grads"} and mats[4].grad is not None
    color, depth, active, frag = r2(*mats)
    color.sum().backward()
    assert set(fake.kw[-1]) == {"camera_grads"}

    # the functional form, and the option's demands
    t = [x.detach() for x in inputs]
    t[0].requires_grad_(True)
    ints = lambda *xs: [x.int() for x in xs]
    call = lambda **kw: dmr.render_tet(t[0], t[1].int(), *t[2:8], *ints(*t[8:11]), settings, **kw)
    out = call(return_fragments=2, fragment_grads=True)
    assert len(out) == 4 and out[3].bary.requires_grad
    out[3].bary.sum().backward()
    assert set(fake.kw[-1]) == {"full_grads", "fragment_grads"} and tuple(fake.kw[-1]["fragment_grads"][1].shape) == (B, 2, 2, H, W)
    with pytest.raises(ValueError, match="return_fragments"):
        dmr.TetRenderer(settings, fragment_grads=True)
    with pytest.raises(ValueError, match="return_fragments"):
        call(fragment_grads=True)
    # a binding that does not know the keyword (tests/standins.py's has no such attribute) is refused at construction
    monkeypatch.setattr(dmr, "_C", _FakeC())
    for make in (lambda: dmr.TetRenderer(settings, return_fragments=2, fragment_grads=True), lambda: call(return_fragments=2, fragment_grads=True)):
        with pytest.raises(TypeError, match="fragment_grads"):
            make()
    assert dmr.TetRenderer(settings, return_fragments=2).return_fragments == 2


def test_sharded_module_refuses_the_option():
    import dmesh_renderer_amd as dmr
    from dmesh_renderer_amd.sharding import ShardedTetRenderer, _Shard
    settings = dmr.TetRenderSettings(32, 32, th.zeros(3), 0)
    with pytest.raises(ValueError, match="sharded"):
        ShardedTetRenderer(settings, impl=object(), fragment_grads=True)
    # ... and so does the Function, whoever hands it a shard
    inputs = [x.detach() for x in _module_inputs(1, 5, 4, 3)]
    with pytest.raises(ValueError, match="sharded"):
        dmr._TetFn.apply(*inputs[:8], *(x.int() for x in inputs[8:]), settings, (0, 0), _Shard(_FragGradFakeC(), None, None), False, False, False, 4, True)


def test_binding_knows_the_keyword_name():
    """All that can be shown without a device: pybind accepts `fragment_grads` as a keyword of render_tets_backward (an unknown
    one is a TypeError) and the call then fails for its CPU tensors, a RuntimeError, before the keyword's own checks -- whose
    messages are tests/test_tet_fragment_grads_gpu.py::test_errors' business."""
    from dmesh_renderer_amd import _C, scenes
    args = scenes.c_args(scenes.kuhn_tets(2, 1, 32, 32), tet=True)
    z = th.zeros(1, dtype=th.uint8)
    with pytest.raises(RuntimeError):
        _C.render_tets_backward(*args, th.zeros(1, 3, 32, 32), th.zeros(1, 1, 32, 32), z, z, z, z,
                                fragment_grads=(th.zeros(1, 2, 32, 32, dtype=th.int32), th.zeros(1, 2, 2, 32, 32)))
    with pytest.raises(TypeError):
        _C.render_tets_backward(*args, th.zeros(1, 3, 32, 32), th.zeros(1, 1, 32, 32), z, z, z, z, no_such_keyword=None)


# ---- the float64 model ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def synthetic():
    d, B, H, W, K, face, gb, pairs, g, dropped = TFG.synthetic()
    return d, B, H, W, K, face, gb, pairs, g, dropped, pairs.grads(g)


def test_synthetic_pairs_of_the_model(synthetic):
    """The pair set of the GPU test: 13 434 pairs (13 440 slots, 6 drew -1), 30 of them with den == 0 exactly (axis-aligned
    Kuhn faces seen edge-on) and 121 (0.9 %, at most 2 %) below the grazing measure 1e-2 and without upstream; (u, v) finite
    on every kept pair."""
    d, B, H, W, K, face, gb, pairs, g, dropped, rg = synthetic
    F = d["faces"].shape[0]
    assert tuple(face.shape) == (B, K, H, W) and face.dtype == th.int32 and int(face.min()) == -1 and int(face.max()) == F - 1
    print(f"\n{len(pairs.u)} pairs, {int((pairs.den == 0).sum())} with den == 0, {int(dropped.sum())} below {TFG.GRAZING_EPS} "
          f"({100 * float(dropped.float().mean()):.2f} %), max |u| {float(pairs.u[~dropped].abs().max()):.3g} "
          f"|v| {float(pairs.v[~dropped].abs().max()):.3g} on the kept ones")
    assert len(pairs.u) == int((face >= 0).sum()) == 13434
    assert int((pairs.den == 0).sum()) == 30 and int(dropped.sum()) == 121 and int(dropped.sum()) <= 0.02 * len(pairs.u)
    assert bool(dropped[pairs.den == 0].all())
    assert bool(th.isfinite(pairs.u[~dropped]).all()) and bool(th.isfinite(pairs.v[~dropped]).all())
    assert bool((g[dropped] == 0).all()) and bool((g[~dropped] != 0).any(1).all())
    assert tuple(gb.shape) == (B, K, 2, H, W) and gb.is_contiguous() and bool((gb[:, :, 0][face < 0] == 0).all())
    # the pairs are not the march's: most rays miss their face
    outside = (pairs.u < 0) | (pairs.v < 0) | (pairs.u + pairs.v > 1)
    assert float(outside[~dropped].float().mean()) > 0.5
    assert all(np.isfinite(x).all() for x in rg.values())
    assert np.abs(rg["verts"]).max() >= 1 and np.abs(rg["mv_mats"]).max() >= 1 and np.abs(rg["proj_mats"]).max() >= 1


def test_model_agrees_with_central_differences(synthetic):
    """Three entries of each leaf: the float64 loss's central differences against autograd, 1e-6 relative."""
    d, B, H, W, K, face, gb, pairs, g, dropped, rg = synthetic
    # the three largest entries of each leaf (a relative bound needs entries that are not zero by construction, as
    # proj_mats[:, 2, 3] is: the rays do not depend on it)
    entries = {k: [tuple(int(i) for i in np.unravel_index(j, rg[k].shape)) for j in np.argsort(-np.abs(rg[k]).ravel())[:3]] for k in TFG.LEAVES}
    for key, idxs in entries.items():
        for idx in idxs:
            fd = TFG.finite_difference(pairs, g, key, idx, h=1e-7)
            ref = float(rg[key][idx])
            e = abs(fd - ref) / max(abs(ref), 1e-30)
            print(f"\n{key}{list(idx)}: autograd {ref:.9g} central difference {fd:.9g} ({e:.1e})")
            assert ref != 0.0 and e <= 1e-6, (key, idx, ref, fd)


def test_float32_autograd_is_well_inside_the_bounds(synthetic):
    """The inputs are fair before any GPU time is spent: the same formula through float32 torch autograd stays under a quarter
    of each bound (measured: verts 5.2e-6, mv_mats 4.4e-6, proj_mats 4.1e-6, max |ref| 5.9e4 / 5.9e4 / 3.7e5)."""
    d, B, H, W, K, face, gb, pairs, g, dropped, rg = synthetic
    r32 = pairs.grads(g, th.float32)
    for key, tol in (("verts", TET_VERTS_TOL), ("mv_mats", MATS_TOL), ("proj_mats", MATS_TOL)):
        big = float(np.abs(rg[key]).max())
        e = float(np.abs(r32[key] - rg[key]).max()) / max(1.0, big)
        print(f"\nfloat32 autograd vs float64, dL_d{key}: {e:.2e} (max |ref| {big:.3g})")
        assert big >= 1.0 and e <= 0.25 * tol, (key, e)
