"""fragments.face_visibility_fused without a GPU: the library exports what include/dmesh_renderer_amd_visibility.h declares,
the binding found it, the torch models (face_visibility with pixel_weight, face_coverage) are what the kernels' definitions
say, and the functional layer refuses what the kernels do not take -- before anything reaches a device."""
import ctypes
import os
import re

import pytest
import torch as th

import dmesh_renderer_amd as dmr
from dmesh_renderer_amd import fragments as FG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dmesh_renderer_amd_visibility.h")
TORCH_PATH = r"fragments\.face_visibility \(and face_coverage\) is the torch path"


def _declared_functions():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(dmr_[a-z_0-9]+)\s*\(", src)))


def test_library_exports_the_declared_symbols():
    from dmesh_renderer_amd import build
    assert _declared_functions() == ["dmr_face_visibility", "dmr_face_visibility_backward"]
    lib = ctypes.CDLL(build.build())
    for n in _declared_functions():
        assert hasattr(lib, n), f"{n} declared in the header but not exported"


def test_the_source_and_header_are_build_dependencies():
    from dmesh_renderer_amd import build
    assert "dmr_visibility.hip" in build.SOURCES and "dmr_deferred_common.hpp" in build.HEADERS   # (its zeroing kernel)
    assert all(os.path.exists(os.path.join(build.CSRC, s)) for s in build.SOURCES)
    for deps in (build.HEADERS, build.GLUE_SOURCES):
        assert any(os.path.basename(d) == "dmesh_renderer_amd_visibility.h" for d in deps)
        assert all(os.path.exists(os.path.join(build.CSRC, d)) for d in deps)


def test_binding_supports_it():
    from dmesh_renderer_amd import _C
    assert _C.SUPPORTS_FRAGMENT_VISIBILITY is True
    assert callable(_C.face_visibility) and callable(_C.face_visibility_backward)
    for n in ("face_visibility", "face_coverage", "face_visibility_fused"):
        assert n in FG.__all__ and callable(getattr(FG, n))
    assert FG._FUSED["face_visibility"] == ("SUPPORTS_FRAGMENT_VISIBILITY", "face-visibility")


# ---------------------------------------------------------------------------
# The torch models
# ---------------------------------------------------------------------------
def _lists(B=2, K=4, H=5, W=6, F=7, seed=0, dtype=th.float64):
    """Random lists with -1 anywhere in them, one opacity exactly 1 and one exactly 0."""
    g = th.Generator().manual_seed(seed)
    face = th.randint(0, F, (B, K, H, W), generator=g, dtype=th.int32)
    face = th.where(th.rand(B, K, H, W, generator=g) < 0.25, th.full_like(face, -1), face)
    opacity = (th.rand(F, generator=g) * 0.6 + 0.05).to(dtype)
    opacity[1], opacity[4] = 1.0, 0.0
    weight = th.randn(B, H, W, generator=g).to(dtype)
    return dmr.Fragments(face, None, None), opacity, weight


def _brute_force(face, opacity, weight, F):
    """The definitions, slot by slot: vis, max_weight, pixels, and sum over pixels of p (1 - T)."""
    B, K, H, W = face.shape
    vis, mx, px, covered = th.zeros(B, F, dtype=th.float64), th.zeros(B, F, dtype=th.float64), th.zeros(B, F, dtype=th.int64), 0.0
    for b in range(B):
        for y in range(H):
            for x in range(W):
                T = 1.0
                for k in range(K):
                    f = int(face[b, k, y, x])
                    if f < 0:
                        continue
                    o = float(opacity[f])
                    w = T * o
                    T *= 1 - o
                    vis[b, f] += float(weight[b, y, x]) * w
                    mx[b, f] = max(float(mx[b, f]), w)
                    px[b, f] += 1
                covered += float(weight[b, y, x]) * (1 - T)
    return vis, mx, px, covered


def test_models_against_a_brute_force_loop():
    """face_visibility with pixel_weight and face_coverage against the definitions; a slot of weight 0 (opacity 0, or behind the
    face of opacity 1) still counts in pixels; without pixel_weight face_visibility is what it was."""
    frag, opacity, weight = _lists()
    F = opacity.shape[0]
    vis_r, mx_r, px_r, covered = _brute_force(frag.pix_to_face, opacity, weight, F)
    vis = FG.face_visibility(frag, opacity, F, weight)
    mx, px = FG.face_coverage(frag, opacity, F)
    assert vis.dtype == th.float64 and tuple(vis.shape) == tuple(mx.shape) == tuple(px.shape) == (2, F)
    assert float((vis - vis_r).abs().max()) <= 1e-12 and float((mx - mx_r).abs().max()) <= 1e-12
    assert px.dtype in (th.int64, th.int32) and th.equal(px.long(), px_r)
    assert int(px[:, 4].min()) > 0 and float(mx[:, 4].max()) == 0.0  # opacity 0: held, never weighted
    assert not mx.requires_grad and not px.requires_grad
    ones = FG.face_visibility(frag, opacity, F, th.ones_like(weight))
    assert th.allclose(FG.face_visibility(frag, opacity, F), ones, rtol=0, atol=1e-14)
    # the sum over the faces: sum over pixels of p (1 - T)
    T = FG._transmittance(FG._opacity_slots(frag, opacity)[1])[:, -1]
    assert abs(float(vis.sum()) - float((weight * (1 - T)).sum())) <= 1e-12
    assert abs(float(vis.sum()) - covered) <= 1e-12


def test_face_coverage_of_a_face_in_no_list():
    frag, opacity, _ = _lists(F=7)
    mx, px = FG.face_coverage(frag, th.cat([opacity, opacity.new_tensor([0.5])]), 8)
    assert float(mx[:, 7].max()) == 0.0 and int(px[:, 7].max()) == 0


def test_gradcheck_of_the_weighted_model():
    frag, opacity, weight = _lists(B=1, K=3, H=3, W=4, F=5, seed=3)
    opacity = opacity.clone().requires_grad_(True)
    weight = weight.clone().requires_grad_(True)
    assert th.autograd.gradcheck(lambda o, p: FG.face_visibility(frag, o, 5, p), (opacity, weight))


# ---------------------------------------------------------------------------
# Refusals, with CPU tensors: nothing reaches a device
# ---------------------------------------------------------------------------
def _inputs(B=1, K=2, H=4, W=5, F=3, dtype=th.float32):
    frag = dmr.Fragments(th.zeros(B, K, H, W, dtype=th.int32), None, None)
    return frag, th.zeros(F, dtype=dtype), th.ones(B, H, W, dtype=dtype)


def test_cpu_tensors_are_refused():
    frag, opacity, weight = _inputs()
    for cov in (False, True):
        with pytest.raises(TypeError, match=r"HIP device.*" + TORCH_PATH):
            FG.face_visibility_fused(frag, opacity, 3, coverage=cov)
    with pytest.raises(TypeError, match=r"HIP device.*" + TORCH_PATH):
        FG.face_visibility_fused(frag, opacity, 3, weight)
    with pytest.raises(RuntimeError, match="no CPU path"):  # the binding below it refuses them too
        dmr._C.face_visibility(frag.pix_to_face, opacity)
    with pytest.raises(RuntimeError, match="no CPU path"):
        dmr._C.face_visibility_backward(frag.pix_to_face, opacity, None, th.zeros(1, 3))


def test_other_dtypes_are_refused():
    frag, opacity, weight = _inputs()
    with pytest.raises(TypeError, match=r"faces_opacity must be float32.*" + TORCH_PATH):
        FG.face_visibility_fused(frag, opacity.double(), 3)
    with pytest.raises(TypeError, match=r"pixel_weight must be float32.*" + TORCH_PATH):
        FG.face_visibility_fused(frag, opacity, 3, weight.double())
    with pytest.raises(TypeError, match=r"pix_to_face must be int32.*" + TORCH_PATH):
        FG.face_visibility_fused(frag._replace(pix_to_face=frag.pix_to_face.long()), opacity, 3)


@pytest.mark.parametrize("K", (0, 33))
def test_k_out_of_range(K):
    frag, opacity, _ = _inputs(K=K)
    with pytest.raises(ValueError, match=rf"K must be in 1\.\.32, got {K}"):
        FG.face_visibility_fused(frag, opacity, 3)


def test_shapes_that_do_not_match():
    frag, opacity, weight = _inputs()
    with pytest.raises(ValueError, match=r"frag\.pix_to_face must be \[B,K,H,W\]"):
        FG.face_visibility_fused(frag._replace(pix_to_face=frag.pix_to_face[0]), opacity, 3)
    with pytest.raises(ValueError, match=r"faces_opacity must be \[F\]"):
        FG.face_visibility_fused(frag, opacity, 4)
    with pytest.raises(ValueError, match=r"faces_opacity must be \[F\]"):
        FG.face_visibility_fused(frag, opacity[:, None], 3)
    for F in (-1, 3.0, None, True):
        with pytest.raises(ValueError, match="F must be a non-negative int"):
            FG.face_visibility_fused(frag, opacity, F)
    for bad in (weight[:, :-1], weight[0], weight.transpose(1, 2), weight[:, None]):
        with pytest.raises(ValueError, match=r"pixel_weight must be \[B,H,W\]"):
            FG.face_visibility_fused(frag, opacity, 3, bad)


def test_a_binding_without_the_calls_says_rebuild(monkeypatch):
    """A `_C` of an older build (no SUPPORTS_FRAGMENT_VISIBILITY, or False): a TypeError that says so, nothing is computed."""
    class Old:
        SUPPORTS_FRAGMENT_COMPOSITE = True
        SUPPORTS_FRAGMENT_TEXTURE = True

    frag, opacity, _ = _inputs()
    monkeypatch.setattr(dmr, "_C", Old())
    with pytest.raises(TypeError, match=r"rebuild.*fragments\.face_visibility is the torch path"):
        FG.face_visibility_fused(frag, opacity, 3)
    Old.SUPPORTS_FRAGMENT_VISIBILITY = False
    with pytest.raises(TypeError, match="rebuild"):
        FG.face_visibility_fused(frag, opacity, 3, coverage=True)
