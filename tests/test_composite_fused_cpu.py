"""fragments.composite_fused without a GPU: the library exports what include/dmesh_renderer_amd_shade.h declares, the binding
found it, and the functional layer refuses what the kernels do not take -- before anything reaches a device."""
import ctypes
import os
import re

import pytest
import torch as th

import dmesh_renderer_amd as dmr
from dmesh_renderer_amd import fragments as FG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dmesh_renderer_amd_shade.h")


def _declared_functions():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(dmr_[a-z_0-9]+)\s*\(", src)))


def test_library_exports_the_declared_symbols():
    from dmesh_renderer_amd import build
    assert _declared_functions() == ["dmr_composite_fragments", "dmr_composite_fragments_backward"]
    lib = ctypes.CDLL(build.build())
    for n in _declared_functions():
        assert hasattr(lib, n), f"{n} declared in the header but not exported"


def test_the_header_is_a_build_dependency():
    from dmesh_renderer_amd import build
    assert "dmr_shade.hip" in build.SOURCES
    for deps in (build.HEADERS, build.GLUE_SOURCES):
        assert any(os.path.basename(d) == "dmesh_renderer_amd_shade.h" for d in deps)
        assert all(os.path.exists(os.path.join(build.CSRC, d)) for d in deps)


def test_binding_supports_it():
    from dmesh_renderer_amd import _C
    assert _C.SUPPORTS_FRAGMENT_COMPOSITE is True
    assert callable(_C.composite_fragments) and callable(_C.composite_fragments_backward)
    assert "composite_fused" in FG.__all__


def _inputs(B=1, K=2, H=4, W=5, P=6, F=3, C=3, dtype=th.float32):
    frag = dmr.Fragments(th.zeros(B, K, H, W, dtype=th.int32), th.zeros(B, K, 2, H, W, dtype=dtype), th.zeros(B, H, W, dtype=th.int32))
    return frag, th.zeros(F, 3, dtype=th.int32), th.zeros(F, dtype=dtype), th.zeros(P, C, dtype=dtype), th.ones(B, F, dtype=dtype)


def test_cpu_tensors_are_refused():
    frag, faces, opacity, attrs, scale = _inputs()
    with pytest.raises(TypeError, match=r"HIP device.*fragments\.composite is the torch path"):
        FG.composite_fused(frag, faces, opacity, attrs)
    with pytest.raises(TypeError, match=r"HIP device.*fragments\.composite is the torch path"):
        FG.composite_fused(frag, faces, opacity, attrs, face_scale=scale)
    with pytest.raises(RuntimeError, match="no CPU path"):  # the binding below it refuses them too
        dmr._C.composite_fragments(frag.pix_to_face, frag.bary, faces, opacity, attrs)


def test_other_dtypes_are_refused():
    frag, faces, opacity, attrs, scale = _inputs(dtype=th.float64)
    with pytest.raises(TypeError, match=r"float32.*fragments\.composite is the torch path"):
        FG.composite_fused(frag, faces, opacity, attrs, face_scale=scale)
    frag, faces, opacity, attrs, scale = _inputs()
    with pytest.raises(TypeError, match=r"face_scale must be float32"):
        FG.composite_fused(frag, faces, opacity, attrs, face_scale=scale.double())
    with pytest.raises(TypeError, match=r"pix_to_face must be int32"):
        FG.composite_fused(frag._replace(pix_to_face=frag.pix_to_face.long()), faces, opacity, attrs)
    with pytest.raises(TypeError, match=r"faces must be an integer tensor"):
        FG.composite_fused(frag, faces.float(), opacity, attrs)


@pytest.mark.parametrize("C", (0, 257))
def test_channel_count_out_of_range(C):
    frag, faces, opacity, attrs, _ = _inputs(C=C)
    with pytest.raises(ValueError, match=r"C must be in 1\.\.256"):
        FG.composite_fused(frag, faces, opacity, attrs)


def test_k_out_of_range():
    frag, faces, opacity, attrs, _ = _inputs(K=33)
    with pytest.raises(ValueError, match=r"K must be in 1\.\.32, got 33"):
        FG.composite_fused(frag, faces, opacity, attrs)


def test_shapes_that_do_not_match():
    frag, faces, opacity, attrs, scale = _inputs()
    with pytest.raises(ValueError, match=r"frag\.bary must be \[B,K,2,H,W\]"):
        FG.composite_fused(frag._replace(bary=frag.bary[:, :1]), faces, opacity, attrs)
    with pytest.raises(ValueError, match=r"frag\.bary must be \[B,K,2,H,W\]"):
        FG.composite_fused(frag._replace(bary=frag.bary.transpose(3, 4)), faces, opacity, attrs)
    with pytest.raises(ValueError, match="faces_opacity"):
        FG.composite_fused(frag, faces, opacity[:-1], attrs)
    with pytest.raises(ValueError, match="face_scale"):
        FG.composite_fused(frag, faces, opacity, attrs, face_scale=scale[:, :-1])


def test_a_binding_without_the_calls_says_rebuild(monkeypatch):
    """A `_C` of an older build (no SUPPORTS_FRAGMENT_COMPOSITE, or False): a TypeError that says so, nothing is computed."""
    class Old:
        pass

    frag, faces, opacity, attrs, _ = _inputs()
    monkeypatch.setattr(dmr, "_C", Old())
    with pytest.raises(TypeError, match="rebuild"):
        FG.composite_fused(frag, faces, opacity, attrs)
    Old.SUPPORTS_FRAGMENT_COMPOSITE = False
    with pytest.raises(TypeError, match="rebuild"):
        FG.composite_fused(frag, faces, opacity, attrs)


def test_torch_functions_are_as_they_were():
    """composite itself is untouched: the model composite_fused is checked against still runs on the CPU, in float64."""
    frag, faces, opacity, attrs, scale = _inputs(dtype=th.float64)
    image, T = FG.composite(frag, faces.long(), opacity + 0.5, attrs + 1.0, face_scale=scale)
    assert image.dtype == th.float64 and tuple(image.shape) == (1, 3, 4, 5) and tuple(T.shape) == (1, 1, 4, 5)
    assert th.allclose(image, th.full_like(image, 0.75)) and th.allclose(T, th.full_like(T, 0.25))
