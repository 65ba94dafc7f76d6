"""fragments.composite_texture / composite_texture_fused without a GPU: the library exports what
include/dmesh_renderer_amd_texture.h declares, the binding found it, the torch model is what its docstring says (gradcheck in
float64, the ramp identity against composite, a 1 x 1 texture), and the fused function refuses what the kernels do not take
-- before anything reaches a device."""
import ctypes
import os
import re

import pytest
import torch as th

import dmesh_renderer_amd as dmr
from dmesh_renderer_amd import fragments as FG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dmesh_renderer_amd_texture.h")


def _declared_functions():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(dmr_[a-z_0-9]+)\s*\(", src)))


def test_library_exports_the_declared_symbols():
    from dmesh_renderer_amd import build
    assert _declared_functions() == ["dmr_composite_texture", "dmr_composite_texture_backward"]
    lib = ctypes.CDLL(build.build())
    for n in _declared_functions():
        assert hasattr(lib, n), f"{n} declared in the header but not exported"


def test_source_and_headers_are_build_dependencies():
    from dmesh_renderer_amd import build
    assert "dmr_texture.hip" in build.SOURCES
    assert "dmr_shade_common.hpp" in build.HEADERS
    for deps in (build.HEADERS, build.GLUE_SOURCES):
        assert any(os.path.basename(d) == "dmesh_renderer_amd_texture.h" for d in deps)
        assert all(os.path.exists(os.path.join(build.CSRC, d)) for d in deps)
    assert all(os.path.exists(os.path.join(build.CSRC, s)) for s in build.SOURCES)


def test_binding_supports_it():
    from dmesh_renderer_amd import _C
    assert _C.SUPPORTS_FRAGMENT_TEXTURE is True
    assert callable(_C.composite_texture) and callable(_C.composite_texture_backward)
    assert "composite_texture" in FG.__all__ and "composite_texture_fused" in FG.__all__


# ---- the model -------------------------------------------------------------------------------------------------------
def _model_inputs(seed, B=2, K=3, H=5, W=6, F=7, Pu=9, C=3, Ht=7, Wt=13, uv_range=(-1.0, 2.0)):
    """float64 lists and leaves; every slot whose sample lies within 1e-3 texel of a texel-centre line is emptied (the UV and
    barycentric gradients jump there: the cell is a constant of the model)."""
    g = th.Generator().manual_seed(seed)
    face = th.randint(-1, F, (B, K, H, W), generator=g, dtype=th.int32)
    bary = th.rand(B, K, 2, H, W, generator=g, dtype=th.float64) * 0.6 - 0.05
    faces = th.randint(0, Pu, (F, 3), generator=g)
    uv_faces = th.randint(0, Pu, (F, 3), generator=g)
    opacity = th.rand(F, generator=g, dtype=th.float64) * 0.6 + 0.01
    uvs = th.rand(Pu, 2, generator=g, dtype=th.float64) * (uv_range[1] - uv_range[0]) + uv_range[0]
    tex = th.randn(Ht, Wt, C, generator=g, dtype=th.float64)
    scale = th.rand(B, F, generator=g, dtype=th.float64) + 0.5
    return dict(face=face, bary=bary, faces=faces, uv_faces=uv_faces, faces_opacity=opacity, vert_uvs=uvs, texture=tex, face_scale=scale)


def _off_the_lines(d, corners, band=1e-3):
    """d["face"] with -1 wherever the slot's x or y lies within `band` of an integer."""
    Ht, Wt, _ = d["texture"].shape
    uv = d["vert_uvs"][corners.long()[d["face"].clamp(min=0).long()]]
    u, v = d["bary"][:, :, 0], d["bary"][:, :, 1]
    st = (th.stack([1 - u - v, u, v], -1).unsqueeze(-1) * uv).sum(-2)
    x, y = st[..., 0] * Wt - 0.5, st[..., 1] * Ht - 0.5
    near = ((x - x.round()).abs() < band) | ((y - y.round()).abs() < band)
    return th.where(near, th.full_like(d["face"], -1), d["face"])


@pytest.mark.parametrize("with_uv_faces", (False, True), ids=("faces", "uv_faces"))
@pytest.mark.parametrize("wrap", FG.WRAPS)
def test_model_gradcheck(wrap, with_uv_faces):
    d = _model_inputs(3 + with_uv_faces)
    corners = d["uv_faces"] if with_uv_faces else d["faces"]
    face = _off_the_lines(d, corners)
    leaves = [d[k].clone().requires_grad_(True) for k in ("bary", "faces_opacity", "vert_uvs", "texture", "face_scale")]

    def fn(bary, opacity, uvs, tex, scale):
        return FG.composite_texture(dmr.Fragments(face, bary, None), d["faces"], opacity, uvs, tex, scale,
                                    uv_faces=corners if with_uv_faces else None, wrap=wrap)

    assert th.autograd.gradcheck(fn, leaves)


@pytest.mark.parametrize("wrap", FG.WRAPS)
def test_ramp_identity(wrap):
    """tex[y, x] = a x + b y, UVs inside [0.5/n, 1 - 0.5/n], uv_faces = None: the bilinear sample of a ramp is the ramp, so the
    result is composite() of the per-vertex attribute a (s Wt - 0.5) + b (t Ht - 0.5)."""
    Ht, Wt = 7, 13
    d = _model_inputs(5, Ht=Ht, Wt=Wt, C=2)
    g = th.Generator().manual_seed(9)
    lo = th.tensor([0.5 / Wt, 0.5 / Ht], dtype=th.float64)
    uvs = lo + th.rand(9, 2, generator=g, dtype=th.float64) * (1 - 2 * lo)
    bary = th.rand(2, 3, 2, 5, 6, generator=g, dtype=th.float64) * 0.5  # inside the face: (s, t) stays inside the UVs' hull
    ab = th.tensor([[0.7, -1.3], [0.25, 2.0]], dtype=th.float64)         # (a, b) per channel
    yy, xx = th.meshgrid(th.arange(Ht, dtype=th.float64), th.arange(Wt, dtype=th.float64), indexing="ij")
    tex = xx.unsqueeze(-1) * ab[:, 0] + yy.unsqueeze(-1) * ab[:, 1]
    attrs = (uvs[:, :1] * Wt - 0.5) * ab[:, 0] + (uvs[:, 1:] * Ht - 0.5) * ab[:, 1]
    frag = dmr.Fragments(d["face"], bary, None)
    image, T = FG.composite_texture(frag, d["faces"], d["faces_opacity"], uvs, tex, d["face_scale"], wrap=wrap)
    image_r, T_r = FG.composite(frag, d["faces"], d["faces_opacity"], attrs, face_scale=d["face_scale"])
    e = float((image - image_r).abs().max())
    print(f"\nramp identity, {wrap}: {e:.2e} (max |image| {float(image_r.abs().max()):.3g})")
    assert float(image_r.abs().max()) > 1 and e <= 1e-13 and th.equal(T, T_r)


def test_one_texel_texture():
    """A 1 x 1 texture: image = sum_k w_k s_k tex[0, 0], whatever the UVs and the wrap, and no UV gradient."""
    d = _model_inputs(7, Ht=1, Wt=1)
    frag = dmr.Fragments(d["face"], d["bary"], None)
    w = FG.blend_weights(frag, d["faces_opacity"])
    s = th.gather(d["face_scale"], 1, d["face"].clamp(min=0).long().reshape(2, -1)).reshape(w.shape)
    expect = (w * s).sum(1, keepdim=True) * d["texture"][0, 0].view(1, -1, 1, 1)
    for wrap in FG.WRAPS:
        uvs = d["vert_uvs"].clone().requires_grad_(True)
        image, _ = FG.composite_texture(frag, d["faces"], d["faces_opacity"], uvs, d["texture"], d["face_scale"], uv_faces=d["uv_faces"], wrap=wrap)
        assert float((image.detach() - expect).abs().max()) <= 1e-14
        image.square().sum().backward()
        assert float(uvs.grad.abs().max()) == 0.0


def test_model_refuses_an_unknown_wrap():
    d = _model_inputs(1)
    with pytest.raises(ValueError, match="wrap"):
        FG.composite_texture(dmr.Fragments(d["face"], d["bary"], None), d["faces"], d["faces_opacity"], d["vert_uvs"], d["texture"], wrap="mirror")


# ---- the fused function's refusals -----------------------------------------------------------------------------------------
def _inputs(B=1, K=2, H=4, W=5, Pu=6, F=3, C=3, Ht=4, Wt=5, dtype=th.float32):
    frag = dmr.Fragments(th.zeros(B, K, H, W, dtype=th.int32), th.zeros(B, K, 2, H, W, dtype=dtype), th.zeros(B, H, W, dtype=th.int32))
    return (frag, th.zeros(F, 3, dtype=th.int32), th.zeros(F, dtype=dtype), th.zeros(Pu, 2, dtype=dtype), th.zeros(Ht, Wt, C, dtype=dtype),
            th.ones(B, F, dtype=dtype))


TORCH_PATH = r"fragments\.composite_texture is the torch path"


def test_cpu_tensors_are_refused():
    frag, faces, opacity, uvs, tex, scale = _inputs()
    with pytest.raises(TypeError, match=r"HIP device.*" + TORCH_PATH):
        FG.composite_texture_fused(frag, faces, opacity, uvs, tex)
    with pytest.raises(TypeError, match=r"HIP device.*" + TORCH_PATH):
        FG.composite_texture_fused(frag, faces, opacity, uvs, tex, scale, uv_faces=faces, wrap="repeat")
    with pytest.raises(RuntimeError, match="no CPU path"):  # the binding below it refuses them too
        dmr._C.composite_texture(frag.pix_to_face, frag.bary, faces, opacity, uvs, tex)


def test_other_dtypes_are_refused():
    frag, faces, opacity, uvs, tex, scale = _inputs(dtype=th.float64)
    with pytest.raises(TypeError, match=r"float32.*" + TORCH_PATH):
        FG.composite_texture_fused(frag, faces, opacity, uvs, tex, scale)
    frag, faces, opacity, uvs, tex, scale = _inputs()
    with pytest.raises(TypeError, match=r"texture must be float32"):
        FG.composite_texture_fused(frag, faces, opacity, uvs, tex.double())
    with pytest.raises(TypeError, match=r"face_scale must be float32"):
        FG.composite_texture_fused(frag, faces, opacity, uvs, tex, scale.double())
    with pytest.raises(TypeError, match=r"pix_to_face must be int32"):
        FG.composite_texture_fused(frag._replace(pix_to_face=frag.pix_to_face.long()), faces, opacity, uvs, tex)
    with pytest.raises(TypeError, match=r"faces must be an integer tensor"):
        FG.composite_texture_fused(frag, faces.float(), opacity, uvs, tex)
    with pytest.raises(TypeError, match=r"uv_faces must be an integer tensor"):
        FG.composite_texture_fused(frag, faces, opacity, uvs, tex, uv_faces=faces.float())


@pytest.mark.parametrize("C", (0, 33))
def test_channel_count_out_of_range(C):
    frag, faces, opacity, uvs, tex, _ = _inputs(C=C)
    with pytest.raises(ValueError, match=r"C must be in 1\.\.32"):
        FG.composite_texture_fused(frag, faces, opacity, uvs, tex)


def test_k_out_of_range():
    frag, faces, opacity, uvs, tex, _ = _inputs(K=33)
    with pytest.raises(ValueError, match=r"K must be in 1\.\.32, got 33"):
        FG.composite_texture_fused(frag, faces, opacity, uvs, tex)


def test_bad_wrap():
    frag, faces, opacity, uvs, tex, _ = _inputs()
    with pytest.raises(ValueError, match=r"wrap must be one of \('clamp', 'repeat'\), got 'mirror'"):
        FG.composite_texture_fused(frag, faces, opacity, uvs, tex, wrap="mirror")


def test_shapes_that_do_not_match():
    frag, faces, opacity, uvs, tex, scale = _inputs()
    with pytest.raises(ValueError, match=r"frag\.bary must be \[B,K,2,H,W\]"):
        FG.composite_texture_fused(frag._replace(bary=frag.bary[:, :1]), faces, opacity, uvs, tex)
    with pytest.raises(ValueError, match="faces_opacity"):
        FG.composite_texture_fused(frag, faces, opacity[:-1], uvs, tex)
    with pytest.raises(ValueError, match="face_scale"):
        FG.composite_texture_fused(frag, faces, opacity, uvs, tex, scale[:, :-1])
    with pytest.raises(ValueError, match="uv_faces"):
        FG.composite_texture_fused(frag, faces, opacity, uvs, tex, uv_faces=faces[:-1])
    with pytest.raises(ValueError, match=r"vert_uvs must be \[Pu,2\]"):
        FG.composite_texture_fused(frag, faces, opacity, th.zeros(6, 3), tex)
    with pytest.raises(ValueError, match=r"texture must be \[Ht,Wt,C\]"):
        FG.composite_texture_fused(frag, faces, opacity, uvs, tex[0])
    with pytest.raises(ValueError, match=r"Ht, Wt >= 1"):
        FG.composite_texture_fused(frag, faces, opacity, uvs, tex[:0])


def test_a_binding_without_the_calls_says_rebuild(monkeypatch):
    """A `_C` of an older build (no SUPPORTS_FRAGMENT_TEXTURE, or False): a TypeError that says so, nothing is computed."""
    class Old:
        SUPPORTS_FRAGMENT_COMPOSITE = True

    frag, faces, opacity, uvs, tex, _ = _inputs()
    monkeypatch.setattr(dmr, "_C", Old())
    with pytest.raises(TypeError, match="rebuild"):
        FG.composite_texture_fused(frag, faces, opacity, uvs, tex)
    Old.SUPPORTS_FRAGMENT_TEXTURE = False
    with pytest.raises(TypeError, match="rebuild"):
        FG.composite_texture_fused(frag, faces, opacity, uvs, tex)
