"""fragment_grads without a GPU: the header's flag and buffer ids, the library's own check of K, the Python plumbing over a
stand-in `_C`, and the float64 model's synthetic pair set (tests/fragment_grads_ref.py) that tests/test_fragment_grads_gpu.py
runs on the device."""
import os
import re

import numpy as np
import pytest
import torch as th

import fragment_grads_ref as FGR
from standins import _StandIn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "dmesh_renderer_amd.h")).read()


def _define(name):
    m = re.search(r"^#define %s(\([a-z]+\))? (.*)$" % name, HEADER, flags=re.M)
    assert m, name
    return m.group(1), m.group(2)


def _macro(name):
    """A function-like macro of the header as a Python function (its body is an integer expression in both languages)."""
    arg, body = _define(name)
    env = {n: int(_define(n)[1]) for n in ("DMR_FLAG_TRI_FRAGMENTS",)}
    return lambda x: eval(body, dict(env, **{arg[1:-1]: x}))


def test_header_defines_the_flag_and_the_two_buffers():
    assert _define("DMR_FLAG_TRI_FRAGMENT_GRADS") == (None, "128")
    assert _define("DMR_ABI_VERSION") == (None, "4")
    assert re.search(r"\bDMR_BUF_TRI_FRAGMENT_FACES = 9\b", HEADER) and re.search(r"\bDMR_BUF_TRI_FRAGMENT_BARY_GRADS = 10\b", HEADER)
    flags = {n: int(_define(n)[1]) for n in re.findall(r"^#define (DMR_FLAG_[A-Z_]+) \d+$", HEADER, flags=re.M)}
    assert len(set(flags.values())) == len(flags) and all(v & (v - 1) == 0 and v < 256 for v in flags.values()), flags


def test_k_stays_readable_next_to_the_flag():
    k_of, flags_of = _macro("DMR_FRAGMENTS_K"), _macro("DMR_FRAGMENTS_FLAGS")
    for k in (1, 2, 8, 32, 255):
        assert k_of(flags_of(k) | 128) == k and k_of(128 | (k << 8)) == k
        assert (flags_of(k) | 128) & 255 == 64 | 128


def test_library_refuses_a_bad_k_before_any_request():
    """dmr_tri_backward with DMR_FLAG_TRI_FRAGMENT_GRADS and K = 0 (or K > 32) fails with a message through dmr_last_error
    before it calls `alloc`; without the flag the K bits are ignored (here: nothing to back-propagate, the call succeeds)."""
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

    def backward(flags, P=3, F=1):
        sc = lib_.Scene(B=1, P=P, F=F, T=0, W=16, H=16, flags=flags)
        return lib.dmr_tri_backward(C.byref(sc), p, p, 0, None, None, None, None, p, p, p, p, p, alloc, None, None)

    for k in (0, 33, 255):
        assert backward(128 | (k << 8)) != 0 and not requested
        msg = lib_.last_error()
        assert "DMR_FLAG_TRI_FRAGMENT_GRADS" in msg and "1..32" in msg and str(k) in msg, msg
    assert backward(128, P=0, F=0) != 0 and not requested  # the check comes first, whatever the scene
    assert backward(33 << 8, P=0, F=0) == 0 and backward(128 | (4 << 8), P=0, F=0) == 0 and not requested


class _FragGradStandIn(_StandIn):
    """tests/standins.py's stand-in with the forward's `fragments` keyword (face ids 0, a bary that is a plain tensor, count 1)."""

    def render_tris(self, *args, rows=(0, 0), **kw):
        H, W = args[11], args[12]
        out = super().render_tris(*args, rows=rows)
        k = kw.get("fragments", 0)
        if k:
            out = out + (th.zeros(self.B, k, H, W, dtype=th.int32), th.full((self.B, k, 2, H, W), 0.25), th.ones(self.B, H, W, dtype=th.int32))
        return out


def _module_inputs(B, P, F):
    g = th.Generator().manual_seed(0)
    eye = th.eye(4, dtype=th.float64).repeat(B, 1, 1)
    return (th.randn(P, 3, generator=g, dtype=th.float64).requires_grad_(True), th.randint(0, P, (F, 3), generator=g),
            th.rand(P, 3, generator=g, dtype=th.float64), th.rand(F, generator=g, dtype=th.float64), eye, eye.clone(),
            th.rand(B, P, generator=g, dtype=th.float64), th.rand(B, F, generator=g, dtype=th.float64))


def test_wrapper_routes_the_keyword_only_with_the_option(monkeypatch):
    import dmesh_renderer_amd as dmr
    B, P, F, H, W, K = 2, 5, 4, 8, 12, 3
    settings = dmr.TriRenderSettings(H, W, th.zeros(3))
    inputs = _module_inputs(B, P, F)
    fake = _FragGradStandIn(B, P, F, H, W, ())
    monkeypatch.setattr(dmr, "_C", fake)

    # without the option: constants, and a backward without the keyword
    color, depth, frag = dmr.TriRenderer(settings, return_fragments=K)(*inputs)
    assert not any(t.requires_grad for t in frag)
    (color.sum() + depth.sum()).backward()
    assert fake.kw[-1] == {}

    # with it: bary is differentiable, face and count are not; the keyword travels only when a gradient for bary arrives
    r = dmr.TriRenderer(settings, return_fragments=K, fragment_grads=True)
    color, depth, frag = r(*inputs)
    assert frag.bary.requires_grad and not frag.pix_to_face.requires_grad and not frag.count.requires_grad
    n = len(fake.kw)
    (color.sum() + depth.sum()).backward()
    assert len(fake.kw) == n + 1 and fake.kw[-1] == {}
    color, depth, frag = r(*inputs)
    up = th.arange(B * K * 2 * H * W, dtype=th.float32).reshape(B, K, 2, H, W)
    inputs[0].grad = None
    (frag.bary * up).sum().backward()
    assert set(fake.kw[-1]) == {"fragment_grads"}
    face, g = fake.kw[-1]["fragment_grads"]
    assert face.dtype == th.int32 and tuple(face.shape) == (B, K, H, W) and th.equal(face, frag.pix_to_face)
    assert g.dtype == th.float32 and g.is_contiguous() and th.equal(g, up)
    assert inputs[0].grad is not None and tuple(inputs[0].grad.shape) == (P, 3)  # (the stand-in's zeros: the verts piece)
    # with the other options the keyword joins theirs
    color, depth, alpha, frag = dmr.TriRenderer(settings, exact_grads=True, return_alpha=True, return_fragments=K, fragment_grads=True)(*inputs)
    (color.sum() + (frag.bary * up).sum()).backward()
    assert set(fake.kw[-1]) == {"exact_grads", "alpha", "fragment_grads"}

    # the functional form, and the option's demands
    t = [x.detach() for x in inputs]
    t[0].requires_grad_(True)
    out = dmr.render_tri(t[0], t[1].int(), *t[2:], settings, return_fragments=2, fragment_grads=True)
    assert len(out) == 3 and out[2].bary.requires_grad
    out[2].bary.sum().backward()
    assert set(fake.kw[-1]) == {"fragment_grads"} and tuple(fake.kw[-1]["fragment_grads"][1].shape) == (B, 2, 2, H, W)
    with pytest.raises(ValueError, match="return_fragments"):
        dmr.TriRenderer(settings, fragment_grads=True)
    with pytest.raises(ValueError, match="return_fragments"):
        dmr.render_tri(t[0], t[1].int(), *t[2:], settings, fragment_grads=True)


def test_sharded_module_refuses_the_option():
    import dmesh_renderer_amd as dmr
    from dmesh_renderer_amd.sharding import ShardedTriRenderer
    with pytest.raises(ValueError, match="sharded"):
        ShardedTriRenderer(dmr.TriRenderSettings(32, 32, th.zeros(3)), impl=object(), fragment_grads=True)


def test_binding_refuses_cpu_tensors_for_the_keyword():
    """The binding has no CPU path at all: the call fails before the keyword is looked at, with a RuntimeError all the same."""
    from dmesh_renderer_amd import _C, scenes
    args = scenes.c_args(scenes.layered_sheets(1, 3, 1, 32, 32))
    z = th.zeros(1, dtype=th.uint8)
    with pytest.raises(RuntimeError):
        _C.render_tris_backward(*args, th.zeros(1, 3, 32, 32), th.zeros(1, 1, 32, 32), 1, z, z, z, z,
                                fragment_grads=(th.zeros(1, 2, 32, 32, dtype=th.int32), th.zeros(1, 2, 2, 32, 32)))


def test_synthetic_pairs_of_the_model():
    """The pair set of the GPU test: 13 413 pairs (13 440 slots, 27 drew -1) over all seven clamp regions, at least 20 in each;
    10 of them (under 5 %) within BORDER_EPS * max(1, |u|, |v|) of a border and without upstream; no non-finite (u, v)."""
    d, B, H, W, K, face, gb, pairs, g, dropped = FGR.synthetic()
    F = d["faces"].shape[0]
    assert tuple(face.shape) == (B, K, H, W) and face.dtype == th.int32 and int(face.min()) == -1 and int(face.max()) == F - 1
    counts = np.bincount(pairs.region.numpy(), minlength=7)
    print(f"\n{len(pairs.u)} pairs, regions {counts.tolist()}, {int(dropped.sum())} near a border "
          f"({int((pairs.border < 1e-4).sum())} within the unscaled 1e-4), max |u| {float(pairs.u.abs().max()):.3g} |v| {float(pairs.v.abs().max()):.3g}")
    assert len(pairs.u) == int((face >= 0).sum()) == 13413
    assert counts.tolist() == [24, 1420, 5471, 5391, 387, 316, 404] and (counts >= 20).all()
    assert int(dropped.sum()) <= 0.05 * len(pairs.u) and int((pairs.border < 1e-4).sum()) == 3
    assert bool(th.isfinite(pairs.u).all()) and bool(th.isfinite(pairs.v).all())
    assert bool((g[dropped] == 0).all()) and bool((g[~dropped] != 0).any(1).all())
    assert tuple(gb.shape) == (B, K, 2, H, W) and bool((gb[:, :, 0][face < 0] == 0).all())
    # the model's region is its clamp's: (u_c, v_c) of every region's formula
    uc, vc = pairs.clamped()
    u, v, r = pairs.u, pairs.v, pairs.region
    want_u = th.where(r == 0, u, th.where((r == 2), th.ones_like(u), th.where(r == 5, u, th.where(r == 6, (1 + u - v) / 2, th.zeros_like(u)))))
    want_v = th.where(r == 0, v, th.where((r == 3), th.ones_like(u), th.where(r == 4, v, th.where(r == 6, (1 - u + v) / 2, th.zeros_like(u)))))
    assert th.equal(uc, want_u) and th.equal(vc, want_v)
    rg = pairs.grads(g)
    assert np.abs(rg["verts"]).max() >= 1 and np.abs(rg["mv_mats"]).max() >= 1 and np.abs(rg["proj_mats"]).max() >= 1
    assert all(np.isfinite(x).all() for x in rg.values())
