"""fragments.interpolate_fused / composite_values_fused without a GPU: the library exports what
include/dmesh_renderer_amd_deferred.h declares, the binding found it, the torch model composite_values is what its definition
says (a brute-force loop, the identity with composite, gradcheck), the functional layer and the C ABI refuse what the kernels
do not take -- before anything reaches a device -- and the case tables of the GPU tests (tests/deferred_cases.py) reach every
kernel instantiation the unit compiles."""
import ctypes as C
import os
import re

import pytest
import torch as th

import deferred_cases as DC
import dmesh_renderer_amd as dmr
from dmesh_renderer_amd import fragments as FG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dmesh_renderer_amd_deferred.h")
UNIT = os.path.join(ROOT, "dmesh_renderer_amd", "csrc", "dmr_interp.hip")
UNIT_TEXT = open(UNIT).read()   # (read at import: every test here is about this unit, and none means anything without it)
COMMON_TEXT = open(os.path.join(ROOT, "dmesh_renderer_amd", "csrc", DC.COMMON_HEADER)).read()   # what it shares with the packed unit
FUNCTIONS = ["dmr_composite_values", "dmr_composite_values_backward", "dmr_interpolate_fragments", "dmr_interpolate_fragments_backward"]


def _declared_functions():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(dmr_[a-z_0-9]+)\s*\(", src)))


def test_library_exports_the_declared_symbols():
    from dmesh_renderer_amd import build
    assert _declared_functions() == FUNCTIONS
    lib = C.CDLL(build.build())
    for n in FUNCTIONS:
        assert hasattr(lib, n), f"{n} declared in the header but not exported"


def test_the_source_and_header_are_build_dependencies():
    from dmesh_renderer_amd import build
    assert "dmr_interp.hip" in build.SOURCES and DC.COMMON_HEADER in build.HEADERS
    assert all(os.path.exists(os.path.join(build.CSRC, s)) for s in build.SOURCES)
    for deps in (build.HEADERS, build.GLUE_SOURCES):
        assert any(os.path.basename(d) == "dmesh_renderer_amd_deferred.h" for d in deps)
        assert all(os.path.exists(os.path.join(build.CSRC, d)) for d in deps)
    assert "dmesh_renderer_amd_deferred.h" in build.__doc__


def test_binding_supports_it():
    from dmesh_renderer_amd import _C
    assert _C.SUPPORTS_FRAGMENT_DEFERRED is True
    for n in ("interpolate_fragments", "interpolate_fragments_backward", "composite_values", "composite_values_backward"):
        assert callable(getattr(_C, n))
    for n in ("composite_values", "interpolate_fused", "composite_values_fused"):
        assert n in FG.__all__ and callable(getattr(FG, n))
    assert FG._FUSED["interpolate"][0] == FG._FUSED["composite_values"][0] == "SUPPORTS_FRAGMENT_DEFERRED"


# ---------------------------------------------------------------------------
# The torch model
# ---------------------------------------------------------------------------
def _lists(B=2, K=4, H=5, W=6, F=7, P=9, Cn=3, seed=0, dtype=th.float64):
    """Random lists with -1 anywhere in them, one opacity exactly 1 and one exactly 0."""
    g = th.Generator().manual_seed(seed)
    face = th.randint(0, F, (B, K, H, W), generator=g, dtype=th.int32)
    face = th.where(th.rand(B, K, H, W, generator=g) < 0.25, th.full_like(face, -1), face)
    bary = (th.rand(B, K, 2, H, W, generator=g) * 0.5).to(dtype)
    opacity = (th.rand(F, generator=g) * 0.6 + 0.05).to(dtype)
    opacity[1], opacity[4 % F] = 1.0, 0.0
    return dict(frag=dmr.Fragments(face, bary, None), faces=th.randint(0, P, (F, 3), generator=g, dtype=th.int32), opacity=opacity,
                values=th.randn(B, K, Cn, H, W, generator=g).to(dtype), scale=(th.rand(B, F, generator=g) + 0.5).to(dtype),
                attrs=th.randn(P, Cn, generator=g).to(dtype))


def _brute_force(face, opacity, values, scale):
    """The definition, slot by slot -> image [B,C,H,W], T [B,1,H,W]."""
    B, K, H, W = face.shape
    Cn = values.shape[2]
    image, Tout = th.zeros(B, Cn, H, W, dtype=th.float64), th.zeros(B, 1, H, W, dtype=th.float64)
    for b in range(B):
        for y in range(H):
            for x in range(W):
                T = 1.0
                for k in range(K):
                    f = int(face[b, k, y, x])
                    if f < 0:
                        continue
                    o = float(opacity[f])
                    w = T * o * (1.0 if scale is None else float(scale[b, f]))
                    T *= 1 - o
                    for c in range(Cn):
                        image[b, c, y, x] += w * float(values[b, k, c, y, x])
                Tout[b, 0, y, x] = T
    return image, Tout


@pytest.mark.parametrize("with_scale", (False, True), ids=("no_scale", "scale"))
def test_composite_values_against_a_brute_force_loop(with_scale):
    """B = 2, K = 4, 5 x 6 pixels, F = 7, -1 anywhere, one opacity exactly 1 and one exactly 0: 1e-12 in float64; a NaN in an
    empty slot's value does not reach the image."""
    d = _lists()
    face, scale = d["frag"].pix_to_face, d["scale"] if with_scale else None
    assert int((face == -1).sum()) > 0 and float(d["opacity"][1]) == 1.0 and float(d["opacity"][4]) == 0.0
    image_r, T_r = _brute_force(face, d["opacity"], d["values"], scale)
    image, T = FG.composite_values(d["frag"], d["opacity"], d["values"], scale)
    assert image.dtype == th.float64 and tuple(image.shape) == (2, 3, 5, 6) and tuple(T.shape) == (2, 1, 5, 6)
    assert float((image - image_r).abs().max()) <= 1e-12 and float((T - T_r).abs().max()) <= 1e-12
    poisoned = th.where((face < 0)[:, :, None].expand_as(d["values"]), th.full_like(d["values"], float("nan")), d["values"])
    assert bool(th.isnan(poisoned).any())
    image_p, T_p = FG.composite_values(d["frag"], d["opacity"], poisoned, scale)
    assert th.equal(image_p, image) and th.equal(T_p, T)
    # float32 in, float32 out
    i32, _ = FG.composite_values(d["frag"], d["opacity"].float(), d["values"].float(), None if scale is None else scale.float())
    assert i32.dtype == th.float32 and float((i32.double() - image_r).abs().max()) <= 1e-5


def test_identity_with_composite():
    """composite_values(frag, o, interpolate(frag, faces, A), s) == composite(frag, faces, o, A, s) to 1e-12 in float64, image and
    T, and the gradients of o, A and s through both sides."""
    d = _lists(seed=1)
    res = []
    for chain in (True, False):
        o, A, s = (d[k].clone().requires_grad_(True) for k in ("opacity", "attrs", "scale"))
        if chain:
            image, T = FG.composite_values(d["frag"], o, FG.interpolate(d["frag"], d["faces"], A), s)
        else:
            image, T = FG.composite(d["frag"], d["faces"], o, A, face_scale=s)
        g = th.Generator().manual_seed(2)
        loss = (image * th.randn(image.shape, generator=g).double()).sum() + (T * th.randn(T.shape, generator=g).double()).sum()
        res.append((image.detach(), T.detach()) + th.autograd.grad(loss, [o, A, s]))
    for name, a, b in zip(("image", "T", "dL_do", "dL_dA", "dL_ds"), *res):
        assert float(b.abs().max()) > 0 and float((a - b).abs().max()) <= 1e-12, name


def test_gradcheck_of_composite_values():
    d = _lists(B=1, K=3, H=3, W=4, F=5, seed=3)
    o, v, s = (d[k].clone().requires_grad_(True) for k in ("opacity", "values", "scale"))
    assert th.autograd.gradcheck(lambda o, v, s: FG.composite_values(d["frag"], o, v, s), (o, v, s))
    assert th.autograd.gradcheck(lambda o, v: FG.composite_values(d["frag"], o, v), (o, v))


# ---------------------------------------------------------------------------
# Refusals of the functional layer, with CPU tensors: nothing reaches a device
# ---------------------------------------------------------------------------
INTERP_PATH = r"fragments\.interpolate is the torch path"
VALUES_PATH = r"fragments\.composite_values is the torch path"


def _inputs(B=1, K=2, H=4, W=5, F=3, P=4, Cn=3):
    frag = dmr.Fragments(th.zeros(B, K, H, W, dtype=th.int32), th.zeros(B, K, 2, H, W), None)
    return dict(frag=frag, faces=th.zeros(F, 3, dtype=th.int32), attrs=th.zeros(P, Cn), opacity=th.zeros(F), values=th.zeros(B, K, Cn, H, W),
                scale=th.ones(B, F))


def test_cpu_tensors_are_refused():
    d = _inputs()
    with pytest.raises(TypeError, match=r"HIP device.*" + INTERP_PATH):
        FG.interpolate_fused(d["frag"], d["faces"], d["attrs"])
    with pytest.raises(TypeError, match=r"HIP device.*" + VALUES_PATH):
        FG.composite_values_fused(d["frag"], d["opacity"], d["values"])
    with pytest.raises(TypeError, match=r"HIP device.*" + VALUES_PATH):
        FG.composite_values_fused(d["frag"]._replace(bary=None), d["opacity"], d["values"], d["scale"])
    with pytest.raises(RuntimeError, match="no CPU path"):  # the binding below it refuses them too
        dmr._C.interpolate_fragments(d["frag"].pix_to_face, d["frag"].bary, d["faces"], d["attrs"])
    with pytest.raises(RuntimeError, match="no CPU path"):
        dmr._C.composite_values(d["frag"].pix_to_face, d["opacity"], d["values"])
    with pytest.raises(RuntimeError, match="no CPU path"):
        dmr._C.interpolate_fragments_backward(d["frag"].pix_to_face, d["frag"].bary, d["faces"], d["attrs"], d["values"])
    with pytest.raises(RuntimeError, match="no CPU path"):
        dmr._C.composite_values_backward(d["frag"].pix_to_face, d["opacity"], d["values"], None, None, None)


def test_other_dtypes_are_refused():
    d = _inputs()
    frag = d["frag"]
    with pytest.raises(TypeError, match=r"vert_attrs must be float32.*" + INTERP_PATH):
        FG.interpolate_fused(frag, d["faces"], d["attrs"].double())
    with pytest.raises(TypeError, match=r"frag\.bary must be float32.*" + INTERP_PATH):
        FG.interpolate_fused(frag._replace(bary=frag.bary.double()), d["faces"], d["attrs"])
    with pytest.raises(TypeError, match=r"pix_to_face must be int32.*" + INTERP_PATH):
        FG.interpolate_fused(frag._replace(pix_to_face=frag.pix_to_face.long()), d["faces"], d["attrs"])
    with pytest.raises(TypeError, match=r"faces must be an integer tensor.*" + INTERP_PATH):
        FG.interpolate_fused(frag, d["faces"].float(), d["attrs"])
    with pytest.raises(TypeError, match=r"values must be float32.*" + VALUES_PATH):
        FG.composite_values_fused(frag, d["opacity"], d["values"].double())
    with pytest.raises(TypeError, match=r"faces_opacity must be float32.*" + VALUES_PATH):
        FG.composite_values_fused(frag, d["opacity"].double(), d["values"])
    with pytest.raises(TypeError, match=r"face_scale must be float32.*" + VALUES_PATH):
        FG.composite_values_fused(frag, d["opacity"], d["values"], d["scale"].double())
    with pytest.raises(TypeError, match=r"pix_to_face must be int32.*" + VALUES_PATH):
        FG.composite_values_fused(frag._replace(pix_to_face=frag.pix_to_face.long()), d["opacity"], d["values"])


@pytest.mark.parametrize("K", (0, 33))
def test_k_out_of_range(K):
    d = _inputs(K=K)
    with pytest.raises(ValueError, match=rf"interpolate_fused: K must be in 1\.\.32, got {K}"):
        FG.interpolate_fused(d["frag"], d["faces"], d["attrs"])
    with pytest.raises(ValueError, match=rf"composite_values_fused: K must be in 1\.\.32, got {K}"):
        FG.composite_values_fused(d["frag"], d["opacity"], d["values"])


@pytest.mark.parametrize("Cn", (0, 257))
def test_c_out_of_range(Cn):
    d = _inputs(Cn=Cn)
    with pytest.raises(ValueError, match=rf"interpolate_fused: C must be in 1\.\.256, got {Cn}"):
        FG.interpolate_fused(d["frag"], d["faces"], d["attrs"])
    with pytest.raises(ValueError, match=rf"composite_values_fused: C must be in 1\.\.256, got {Cn}"):
        FG.composite_values_fused(d["frag"], d["opacity"], d["values"])


def test_shapes_that_do_not_match():
    d = _inputs()
    frag, v = d["frag"], d["values"]
    with pytest.raises(ValueError, match=r"frag\.pix_to_face must be \[B,K,H,W\]"):
        FG.interpolate_fused(frag._replace(pix_to_face=frag.pix_to_face[0]), d["faces"], d["attrs"])
    with pytest.raises(ValueError, match=r"frag\.bary must be \[B,K,2,H,W\]"):
        FG.interpolate_fused(frag._replace(bary=frag.bary[:, :, :1]), d["faces"], d["attrs"])
    with pytest.raises(ValueError, match=r"frag\.bary must be \[B,K,2,H,W\].*got None"):
        FG.interpolate_fused(frag._replace(bary=None), d["faces"], d["attrs"])
    with pytest.raises(ValueError, match=r"faces must be \[F,3\]"):
        FG.interpolate_fused(frag, d["faces"][:, :2], d["attrs"])
    with pytest.raises(ValueError, match=r"vert_attrs must be \[P,C\]"):
        FG.interpolate_fused(frag, d["faces"], d["attrs"][0])
    with pytest.raises(ValueError, match=r"frag\.pix_to_face must be \[B,K,H,W\]"):
        FG.composite_values_fused(frag._replace(pix_to_face=frag.pix_to_face[0]), d["opacity"], v)
    with pytest.raises(ValueError, match=r"faces_opacity must be \[F\]"):
        FG.composite_values_fused(frag, d["opacity"][:, None], v)
    for bad in (v[0], v[:, :1], v[:, :, :, :-1], v.permute(0, 2, 1, 3, 4), v.permute(0, 1, 3, 4, 2)):
        with pytest.raises(ValueError, match=r"values must be \[B,K,C,H,W\]"):
            FG.composite_values_fused(frag, d["opacity"], bad)
    for bad in (d["scale"][:, :-1], d["scale"][0], d["scale"].t()):
        with pytest.raises(ValueError, match=r"face_scale must be \[B,F\]"):
            FG.composite_values_fused(frag, d["opacity"], v, bad)


def test_a_binding_without_the_calls_says_rebuild(monkeypatch):
    """A `_C` of an older build (no SUPPORTS_FRAGMENT_DEFERRED, or False): a TypeError that says so, nothing is computed."""
    class Old:
        SUPPORTS_FRAGMENT_COMPOSITE = True
        SUPPORTS_FRAGMENT_TEXTURE = True
        SUPPORTS_FRAGMENT_VISIBILITY = True

    d = _inputs()
    monkeypatch.setattr(dmr, "_C", Old())
    with pytest.raises(TypeError, match=r"interpolate_fused.*no fused fragment interpolation: rebuild.*" + INTERP_PATH):
        FG.interpolate_fused(d["frag"], d["faces"], d["attrs"])
    with pytest.raises(TypeError, match=r"composite_values_fused.*no fused per-slot value compositing: rebuild.*" + VALUES_PATH):
        FG.composite_values_fused(d["frag"], d["opacity"], d["values"])
    Old.SUPPORTS_FRAGMENT_DEFERRED = False
    with pytest.raises(TypeError, match="rebuild"):
        FG.interpolate_fused(d["frag"], d["faces"], d["attrs"])


# ---------------------------------------------------------------------------
# Refusals of the C ABI, through ctypes with pointers that are never dereferenced (as tests/test_shading_refusals_cpu.py): every
# check runs before any HIP call.  No call here has wholly valid arguments and an output to write: none reaches a launch.
# ---------------------------------------------------------------------------
D = C.c_void_p(16)  # non-null, never dereferenced on these paths
INT_MAX = 2 ** 31 - 1
CALLS = {
    "dmr_interpolate_fragments": ("B K H W P F C", "face bary faces vert_attrs out stream"),
    "dmr_interpolate_fragments_backward": ("B K H W P F C", "face bary faces vert_attrs grad_out dL_dvert_attrs dL_dbary stream"),
    "dmr_composite_values": ("B K H W F C", "face faces_opacity values face_scale image T stream"),
    "dmr_composite_values_backward": ("B K H W F C", "face faces_opacity values face_scale grad_image grad_T dL_dfaces_opacity dL_dvalues "
                                      "dL_dface_scale stream"),
}
SIZES = dict(B=1, K=1, H=1, W=1, P=3, F=1, C=3)
NULL_BY_DEFAULT = ("face_scale", "stream", "dL_dvert_attrs", "dL_dbary", "dL_dfaces_opacity", "dL_dvalues", "dL_dface_scale")

# case -> (the arguments it changes, the text after "<call>: "; None: the call returns 0); a case that names an argument a call
# does not take is skipped for that call
EVERY_CALL = {
    "B=0": (dict(B=0), "bad dimensions"), "H=0": (dict(H=0), "bad dimensions"), "W=0": (dict(W=0), "bad dimensions"),
    "F<0": (dict(F=-1), "bad dimensions"), "P<0": (dict(P=-1), "bad dimensions"),
    "K=0": (dict(K=0), "K must be in 1..32, got 0"), "K=33": (dict(K=33), "K must be in 1..32, got 33"),
    "C=0": (dict(C=0), "C must be in 1..256, got 0"), "C=257": (dict(C=257), "C must be in 1..256, got 257"),
    "null face": (dict(face=None), "null fragment lists"), "null bary": (dict(bary=None), "null fragment lists"),
    "null faces": (dict(faces=None), "null faces"), "null vert_attrs": (dict(vert_attrs=None), "null vert_attrs"),
    "null faces_opacity": (dict(faces_opacity=None), "null faces_opacity"), "null values": (dict(values=None), "null values"),
    "tiles >= 2^31": (dict(B=INT_MAX, H=17, W=17), "problem too large"), "B F >= 2^31": (dict(B=65536, F=65536), "problem too large"),
    "K H W >= 2^31": (dict(K=32, H=65536, W=1024), "problem too large"),
    # two at once: the first check wins
    "bad K and bad C": (dict(K=0, C=0), "K must be in 1..32, got 0"), "bad C and null lists": (dict(C=0, face=None), "C must be in 1..256, got 0"),
    "bad dimensions and bad K": (dict(W=0, K=99), "bad dimensions"),
    "null lists and null table": (dict(face=None, faces=None, faces_opacity=None), "null fragment lists"),
    "null table and too large": (dict(faces=None, faces_opacity=None, B=65536, F=65536), ("null faces", "null faces_opacity")),
}
PER_CALL = {
    "dmr_interpolate_fragments": {"null out": (dict(out=None), "null output"),
                                  "no faces, no table, null out": (dict(F=0, faces=None, vert_attrs=None, out=None), "null output")},
    "dmr_interpolate_fragments_backward": {"null grad_out": (dict(grad_out=None), "null grad_out"), "no gradient wanted": (dict(), None),
                                           "bad K although no gradient wanted": (dict(K=0), "K must be in 1..32, got 0"),
                                           "null grad_out and no gradient wanted": (dict(grad_out=None), "null grad_out")},
    "dmr_composite_values": {"null image": (dict(image=None), "null output"), "null T": (dict(T=None), "null output"),
                             "no faces, no opacities, null image": (dict(F=0, faces_opacity=None, image=None), "null output")},
    "dmr_composite_values_backward": {"dL_dface_scale without face_scale": (dict(dL_dface_scale=D), "dL_dface_scale without face_scale"),
                                      "no gradient wanted": (dict(), None), "no gradient wanted, no upstream": (dict(grad_image=None, grad_T=None), None),
                                      "bad K although no gradient wanted": (dict(K=0), "K must be in 1..32, got 0"),
                                      "null values and dL_dface_scale without face_scale": (dict(values=None, dL_dface_scale=D), "null values")},
}


def _library():
    import capi_ctypes
    lib = capi_ctypes.load()
    for call, (ints, ptrs) in CALLS.items():
        fn = getattr(lib, call)
        fn.restype = C.c_int
        fn.argtypes = [C.c_int] * len(ints.split()) + [C.c_void_p] * len(ptrs.split())
    return lib


def _refusal_cases():
    for call, (ints, ptrs) in CALLS.items():
        takes = ints.split() + ptrs.split()
        for case, (changes, text) in list(EVERY_CALL.items()) + list(PER_CALL[call].items()):
            if all(k in takes for k in changes) or case.startswith(("null lists and", "null table and")):
                yield call, case, {k: v for k, v in changes.items() if k in takes}, text


def test_c_abi_refusals():
    lib = _library()
    seen = set()
    for call, case, changes, text in _refusal_cases():
        ints, ptrs = CALLS[call]
        args = [changes.get(n, SIZES[n]) for n in ints.split()] + [changes.get(n, None if n in NULL_BY_DEFAULT else D) for n in ptrs.split()]
        ret = getattr(lib, call)(*args)
        got = lib.dmr_last_error().decode() if ret else ""
        if text is None:
            assert (ret, got) == (0, ""), (call, case, got)
        else:
            want = [f"{call}: {t}" for t in ((text,) if isinstance(text, str) else text)]
            assert ret == 1 and got in want, (call, case, got)
        seen.add((call, case))
    # every size check, the null lists, the null tables, the null outputs, the prologue and the pairs were tripped in every call they apply to
    for call in CALLS:
        for case in ("B=0", "H=0", "W=0", "F<0", "K=0", "K=33", "C=0", "C=257", "null face", "tiles >= 2^31", "B F >= 2^31", "K H W >= 2^31",
                     "bad K and bad C", "bad C and null lists", "bad dimensions and bad K", "null lists and null table", "null table and too large"):
            assert (call, case) in seen, (call, case)
        assert all((call, case) in seen for case in PER_CALL[call])
    assert ("dmr_interpolate_fragments", "P<0") in seen and ("dmr_interpolate_fragments_backward", "null vert_attrs") in seen
    assert ("dmr_composite_values", "null values") in seen and ("dmr_composite_values", "P<0") not in seen


# ---------------------------------------------------------------------------
# The case tables of the GPU tests
# ---------------------------------------------------------------------------
def _all_cases():
    return [r for rows in DC.tables().values() for r in rows]


def test_dispatch_restated_as_the_unit_has_it():
    unit = UNIT_TEXT
    for line in DC.DISPATCH_LINES:
        assert unit.count(line) == 1 and COMMON_TEXT.count(line) == 0, line
    for line in DC.COMMON_DISPATCH_LINES:
        assert COMMON_TEXT.count(line) == 1 and unit.count(line) == 0, line
    assert '#include "%s"' % DC.COMMON_HEADER in unit
    assert [DC.interp_ch(c) for c in (1, 4, 5, 256)] == [4, 4, 8, 8]
    assert [DC.values_forward_ch(c) for c in (1, 4, 5, 256)] == [4, 4, 16, 16]
    assert [DC.values_backward_ch(c) for c in (1, 4, 5, 256)] == [4, 4, 8, 8]
    # the kernels the unit instantiates are the ones every_instantiation lists
    named = set(re.findall(r"\b(k_[a-z_]+)<", unit))   # (k_deferred_zero is the common header's)
    assert named == {k for k, _, _ in DC.every_instantiation()}


def test_tables_reach_every_instantiation():
    full = DC.every_instantiation()
    assert len(full) == 4 + 4 + 2 + 8
    reached = DC.instantiations(_all_cases())
    assert reached == full, sorted(full - reached, key=str)


def test_every_kmax_at_its_ends():
    ks = {r.K for r in _all_cases()}
    for kmax in DC.KMAXES:
        assert kmax in ks and DC.smallest_k(kmax) in ks, kmax
        for ch in (4, 8):  # ... with either channel chunk
            assert any(r.K == kmax and DC.values_backward_ch(r.C) == ch for r in _all_cases()), (kmax, ch)
    cs = {r.C for r in _all_cases()}
    assert {1, 4, 8, 16, 20, 255, 256} <= cs
    assert any(r.C % 4 == 0 and not r.aligned and r.C <= 4 for r in _all_cases()) and any(r.C % 4 == 0 and not r.aligned and r.C > 4 for r in _all_cases())


def test_gpu_cases_have_non_zero_references():
    """Every GPU case that compares against a float64 model: a non-zero reference for the outputs and for every gradient."""
    import test_deferred_gpu as G
    n = 0
    for tag, refs in G.all_cases():
        G.check_inputs(refs)
        n += 1
    print(f"\n{n} references")
    assert n == 3 * len(DC.LISTS_K) * len(DC.LISTS_C) * len(DC.SIZES) + 2 * len(DC.MATRIX) + 2 * len(DC.EDGE_FRAMES) + 2
