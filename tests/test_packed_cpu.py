"""fragments.pack_slots / interpolate_packed / composite_values_packed and their fused forms without a GPU: the library exports
what include/dmesh_renderer_amd_packed.h declares, the binding found it, the torch models are what their definitions say (a
brute-force loop for the packing, the two identities with the dense models to 1e-12 in float64, gradcheck), the functional
layer and the C ABI refuse what the kernels do not take -- before anything reaches a device -- and the case tables of the GPU
tests (tests/packed_cases.py) reach every kernel instantiation the unit compiles."""
import ctypes as C
import os
import re

import pytest
import torch as th

import packed_cases as PC
import dmesh_renderer_amd as dmr
from dmesh_renderer_amd import fragments as FG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dmesh_renderer_amd_packed.h")
UNIT = os.path.join(ROOT, "dmesh_renderer_amd", "csrc", "dmr_packed.hip")
UNIT_TEXT = open(UNIT).read()   # (read at import: every test here is about this unit, and none means anything without it)
COMMON_TEXT = open(os.path.join(ROOT, "dmesh_renderer_amd", "csrc", PC.COMMON_HEADER)).read()   # what it shares with the dense unit
FUNCTIONS = ["dmr_composite_values_packed", "dmr_composite_values_packed_backward", "dmr_interpolate_packed",
             "dmr_interpolate_packed_backward", "dmr_pack_slots"]
NAMES = ("PackedSlots", "pack_slots", "pack_slots_fused", "interpolate_packed", "interpolate_packed_fused", "composite_values_packed",
         "composite_values_packed_fused", "unpack_values")


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
    assert "dmr_packed.hip" in build.SOURCES and PC.COMMON_HEADER in build.HEADERS
    assert all(os.path.exists(os.path.join(build.CSRC, s)) for s in build.SOURCES)
    for deps in (build.HEADERS, build.GLUE_SOURCES):
        assert any(os.path.basename(d) == "dmesh_renderer_amd_packed.h" for d in deps)
        assert all(os.path.exists(os.path.join(build.CSRC, d)) for d in deps)
    assert "dmesh_renderer_amd_packed.h" in build.__doc__


def test_binding_supports_it():
    from dmesh_renderer_amd import _C
    assert _C.SUPPORTS_FRAGMENT_PACKED is True
    for n in ("pack_slots", "interpolate_packed", "interpolate_packed_backward", "composite_values_packed", "composite_values_packed_backward"):
        assert callable(getattr(_C, n))
    for n in NAMES:
        assert n in FG.__all__ and callable(getattr(FG, n))
    assert {FG._FUSED[k][0] for k in ("pack_slots", "interpolate_packed", "composite_values_packed")} == {"SUPPORTS_FRAGMENT_PACKED"}
    assert _C.ABI_VERSION == 4 and _C.NUM_STAGES == 12   # (the header adds calls, not a version)


# ---------------------------------------------------------------------------
# The torch models
# ---------------------------------------------------------------------------
def _lists(B=2, K=4, H=5, W=6, F=7, P=9, Cn=3, seed=0, dtype=th.float64):
    """Random lists with -1 anywhere in them and ids past F, one opacity exactly 1 and one exactly 0."""
    g = th.Generator().manual_seed(seed)
    face = th.randint(0, F, (B, K, H, W), generator=g, dtype=th.int32)
    r = th.rand(B, K, H, W, generator=g)
    face = th.where(r < 0.2, th.full_like(face, -1), face)
    face = th.where((r >= 0.2) & (r < 0.3), face + F + (face % 3) * 5, face)
    bary = (th.rand(B, K, 2, H, W, generator=g) * 0.5).to(dtype)
    opacity = (th.rand(F, generator=g) * 0.6 + 0.05).to(dtype)
    opacity[1], opacity[4 % F] = 1.0, 0.0
    return dict(frag=dmr.Fragments(face, bary, None), faces=th.randint(0, P, (F, 3), generator=g, dtype=th.int32), opacity=opacity,
                scale=(th.rand(B, F, generator=g) + 0.5).to(dtype), attrs=th.randn(P, Cn, generator=g).to(dtype), F=F, Cn=Cn, seed=seed)


def _brute_force_pack(face, F, capacity):
    """The definition, slot by slot in the order of face.flatten() -> row (list), n_used, rows."""
    row, n = [], 0
    for f in face.flatten().tolist():
        used = 0 <= f < F
        row.append(n if used and (capacity is None or n < capacity) else -1)
        n += used
    return row, n, n if capacity is None else capacity


@pytest.mark.parametrize("fill", ("mixed", "all_empty", "all_used"))
def test_pack_slots_against_a_brute_force_loop(fill):
    """-1 anywhere, ids past F; all empty; all used; capacity None, 0, below, equal to and above the count."""
    d = _lists()
    face, F = d["frag"].pix_to_face, d["F"]
    if fill == "all_empty":
        face = th.where(face % 2 == 0, th.full_like(face, -1), face.clamp(min=0) + F)
    elif fill == "all_used":
        face = face.clamp(min=0) % F
    frag = dmr.Fragments(face, None, None)
    count = int(((face >= 0) & (face < F)).sum())
    assert (count == 0) == (fill == "all_empty") and (count == face.numel()) == (fill == "all_used")
    for capacity in (None, 0, max(count - 7, 0), count, count + 5):
        row_r, n_r, rows_r = _brute_force_pack(face, F, capacity)
        p = FG.pack_slots(frag, F, capacity)
        assert isinstance(p, FG.PackedSlots) and p.row.dtype == p.n_used.dtype == th.int32 and tuple(p.n_used.shape) == (1,)
        assert tuple(p.row.shape) == tuple(face.shape) and isinstance(p.rows, int)
        assert p.row.flatten().tolist() == row_r and int(p.n_used) == n_r == count and p.rows == rows_r, (fill, capacity)
    for bad in (-1, 1.5, True):
        with pytest.raises(ValueError, match="capacity must be None or a non-negative int"):
            FG.pack_slots(frag, F, bad)
    with pytest.raises(ValueError, match="F must be a non-negative int"):
        FG.pack_slots(frag, -1)


def _dropped(frag, packed, F):
    """frag with every slot that does not count set to -1."""
    face = frag.pix_to_face
    live = (packed.row >= 0) & (packed.row < packed.rows) & (face >= 0) & (face < F)
    return frag._replace(pix_to_face=th.where(live, face, th.full_like(face, -1)))


@pytest.mark.parametrize("capacity", (None, "below", "above"))
def test_the_two_identities(capacity):
    """interpolate_packed == interpolate(...).permute(0, 1, 3, 4, 2)[row >= 0] reordered by row (zeros in the other rows), and
    composite_values_packed(v) == composite_values(frag', o, unpack_values(v), s), to 1e-12 in float64, with the gradients of A,
    bary, o, values and s through both sides."""
    d = _lists(seed=1)
    frag, F, Cn = d["frag"], d["F"], d["Cn"]
    count = int(((frag.pix_to_face >= 0) & (frag.pix_to_face < F)).sum())
    cap = {None: None, "below": count - 20, "above": count + 9}[capacity]
    packed = FG.pack_slots(frag, F, cap)
    N = packed.rows
    g = th.Generator().manual_seed(2)
    g_rows, values = th.randn(N, Cn, generator=g).double(), th.randn(N, Cn, generator=g).double()
    g_image, g_T = th.randn(2, Cn, 5, 6, generator=g).double(), th.randn(2, 1, 5, 6, generator=g).double()
    held = packed.row >= 0
    assert int(held.sum()) == min(count, N) and bool((packed.row[held] == th.arange(int(held.sum()), dtype=th.int32)).all())  # in flat order
    res = []
    for side in ("packed", "dense"):
        A, bary = d["attrs"].clone().requires_grad_(True), frag.bary.clone().requires_grad_(True)
        fr = frag._replace(bary=bary)
        if side == "packed":
            out = FG.interpolate_packed(fr, packed, d["faces"], A)
        else:
            rows = FG.interpolate(_dropped(fr, packed, F), d["faces"], A).permute(0, 1, 3, 4, 2)[held]
            out = th.cat([rows, rows.new_zeros(N - rows.shape[0], Cn)])
        res.append((out.detach(),) + th.autograd.grad((out * g_rows).sum(), [A, bary]))
    for name, a, b in zip(("out", "dL_dA", "dL_dbary"), *res):
        assert float(b.abs().max()) > 0 and float((a - b).abs().max()) <= 1e-12, name
    assert tuple(res[0][0].shape) == (N, Cn) and float(res[0][0][min(count, N):].abs().max() if N > count else 0.0) == 0.0
    assert float(res[0][2][:, :, :1][~held[:, :, None]].abs().max()) == 0.0   # dL_dbary: 0 in empty and dropped slots
    res = []
    for side in ("packed", "dense"):
        o, v, s = (x.clone().requires_grad_(True) for x in (d["opacity"], values, d["scale"]))
        if side == "packed":
            image, T = FG.composite_values_packed(frag, packed, o, v, s)
        else:
            image, T = FG.composite_values(_dropped(frag, packed, F), o, FG.unpack_values(frag, packed, v), s)
        res.append((image.detach(), T.detach()) + th.autograd.grad((image * g_image).sum() + (T * g_T).sum(), [o, v, s]))
    for name, a, b in zip(("image", "T", "dL_do", "dL_dvalues", "dL_ds"), *res):
        assert float(b.abs().max()) > 0 and float((a - b).abs().max()) <= 1e-12, name
    if N > count:
        assert float(res[0][3][count:].abs().max()) == 0.0
    # unpack_values: the slot's row, 0 where there is none
    u = FG.unpack_values(frag, packed, values)
    assert tuple(u.shape) == (2, 4, Cn, 5, 6) and float(u.permute(0, 1, 3, 4, 2)[~held].abs().max()) == 0.0
    assert th.equal(u.permute(0, 1, 3, 4, 2)[held], values[:int(held.sum())])


def test_a_packed_made_for_a_larger_f():
    """Slots with a row whose face id is outside the call's [0, F): rows of zeros, skipped by the blend, zeros in dL_dvalues."""
    d = _lists(seed=4)
    frag, F = d["frag"], d["F"]
    packed = FG.pack_slots(frag, F + 6)
    extra = (frag.pix_to_face >= F) & (packed.row >= 0)
    assert int(extra.sum()) > 0
    out = FG.interpolate_packed(frag, packed, d["faces"], d["attrs"])
    assert float(out[packed.row[extra].long()].abs().max()) == 0.0 and float(out.abs().max()) > 0
    v = th.randn(packed.rows, 3, dtype=th.float64).requires_grad_(True)
    image, T = FG.composite_values_packed(frag, packed, d["opacity"], v)
    image_r, T_r = FG.composite_values(_dropped(frag, packed, F), d["opacity"], FG.unpack_values(frag, packed, v))
    assert th.equal(image, image_r) and th.equal(T, T_r)
    gv, = th.autograd.grad(image.sum(), v)
    assert float(gv[packed.row[extra].long()].abs().max()) == 0.0 and float(gv.abs().max()) > 0


def test_gradcheck_of_the_packed_models():
    d = _lists(B=1, K=3, H=3, W=4, F=5, seed=3)
    frag, F = d["frag"], d["F"]
    for cap in (None, 9):
        packed = FG.pack_slots(frag, F, cap)
        A, bary = d["attrs"].clone().requires_grad_(True), frag.bary.clone().requires_grad_(True)
        assert th.autograd.gradcheck(lambda A, bary: FG.interpolate_packed(frag._replace(bary=bary), packed, d["faces"], A), (A, bary))
        o, s = d["opacity"].clone().requires_grad_(True), d["scale"].clone().requires_grad_(True)
        v = th.randn(packed.rows, 3, dtype=th.float64, generator=th.Generator().manual_seed(5)).requires_grad_(True)
        assert th.autograd.gradcheck(lambda o, v, s: FG.composite_values_packed(frag, packed, o, v, s), (o, v, s))
        assert th.autograd.gradcheck(lambda o, v: FG.composite_values_packed(frag, packed, o, v), (o, v))


# ---------------------------------------------------------------------------
# Refusals of the functional layer, with CPU tensors: nothing reaches a device
# ---------------------------------------------------------------------------
PACK_PATH = r"fragments\.pack_slots is the torch path"
INTERP_PATH = r"fragments\.interpolate_packed is the torch path"
VALUES_PATH = r"fragments\.composite_values_packed is the torch path"


def _inputs(B=1, K=2, H=4, W=5, F=3, P=4, Cn=3, N=6):
    frag = dmr.Fragments(th.zeros(B, K, H, W, dtype=th.int32), th.zeros(B, K, 2, H, W), None)
    packed = FG.PackedSlots(th.zeros(B, K, H, W, dtype=th.int32), th.zeros(1, dtype=th.int32), N)
    return dict(frag=frag, packed=packed, faces=th.zeros(F, 3, dtype=th.int32), attrs=th.zeros(P, Cn), opacity=th.zeros(F), values=th.zeros(N, Cn),
                scale=th.ones(B, F), F=F)


def test_cpu_tensors_are_refused():
    d = _inputs()
    with pytest.raises(TypeError, match=r"HIP device.*" + PACK_PATH):
        FG.pack_slots_fused(d["frag"], d["F"])
    with pytest.raises(TypeError, match=r"HIP device.*" + PACK_PATH):
        FG.pack_slots_fused(d["frag"], d["F"], capacity=4)
    with pytest.raises(TypeError, match=r"HIP device.*" + INTERP_PATH):
        FG.interpolate_packed_fused(d["frag"], d["packed"], d["faces"], d["attrs"])
    with pytest.raises(TypeError, match=r"HIP device.*" + VALUES_PATH):
        FG.composite_values_packed_fused(d["frag"], d["packed"], d["opacity"], d["values"])
    with pytest.raises(TypeError, match=r"HIP device.*" + VALUES_PATH):
        FG.composite_values_packed_fused(d["frag"]._replace(bary=None), d["packed"], d["opacity"], d["values"], d["scale"])
    f, p = d["frag"], d["packed"]
    for call in (lambda: dmr._C.pack_slots(f.pix_to_face, 3, 4),
                 lambda: dmr._C.interpolate_packed(f.pix_to_face, f.bary, p.row, p.n_used, d["faces"], d["attrs"], 6),
                 lambda: dmr._C.interpolate_packed_backward(f.pix_to_face, f.bary, p.row, p.n_used, d["faces"], d["attrs"], d["values"]),
                 lambda: dmr._C.composite_values_packed(f.pix_to_face, p.row, d["opacity"], d["values"]),
                 lambda: dmr._C.composite_values_packed_backward(f.pix_to_face, p.row, p.n_used, d["opacity"], d["values"], None, None, None)):
        with pytest.raises(RuntimeError, match="no CPU path"):  # the binding below it refuses them too
            call()


def test_other_dtypes_are_refused():
    d = _inputs()
    frag, packed = d["frag"], d["packed"]
    with pytest.raises(TypeError, match=r"pix_to_face must be int32.*" + PACK_PATH):
        FG.pack_slots_fused(frag._replace(pix_to_face=frag.pix_to_face.long()), d["F"])
    with pytest.raises(TypeError, match=r"vert_attrs must be float32.*" + INTERP_PATH):
        FG.interpolate_packed_fused(frag, packed, d["faces"], d["attrs"].double())
    with pytest.raises(TypeError, match=r"frag\.bary must be float32.*" + INTERP_PATH):
        FG.interpolate_packed_fused(frag._replace(bary=frag.bary.double()), packed, d["faces"], d["attrs"])
    with pytest.raises(TypeError, match=r"pix_to_face must be int32.*" + INTERP_PATH):
        FG.interpolate_packed_fused(frag._replace(pix_to_face=frag.pix_to_face.long()), packed, d["faces"], d["attrs"])
    with pytest.raises(TypeError, match=r"faces must be an integer tensor.*" + INTERP_PATH):
        FG.interpolate_packed_fused(frag, packed, d["faces"].float(), d["attrs"])
    with pytest.raises(TypeError, match=r"packed\.row must be int32.*" + INTERP_PATH):
        FG.interpolate_packed_fused(frag, packed._replace(row=packed.row.long()), d["faces"], d["attrs"])
    with pytest.raises(TypeError, match=r"packed\.n_used must be int32.*" + INTERP_PATH):
        FG.interpolate_packed_fused(frag, packed._replace(n_used=packed.n_used.long()), d["faces"], d["attrs"])
    with pytest.raises(TypeError, match=r"values must be float32.*" + VALUES_PATH):
        FG.composite_values_packed_fused(frag, packed, d["opacity"], d["values"].double())
    with pytest.raises(TypeError, match=r"faces_opacity must be float32.*" + VALUES_PATH):
        FG.composite_values_packed_fused(frag, packed, d["opacity"].double(), d["values"])
    with pytest.raises(TypeError, match=r"face_scale must be float32.*" + VALUES_PATH):
        FG.composite_values_packed_fused(frag, packed, d["opacity"], d["values"], d["scale"].double())
    with pytest.raises(TypeError, match=r"packed\.row must be int32.*" + VALUES_PATH):
        FG.composite_values_packed_fused(frag, packed._replace(row=packed.row.long()), d["opacity"], d["values"])
    with pytest.raises(TypeError, match=r"pix_to_face must be int32.*" + VALUES_PATH):
        FG.composite_values_packed_fused(frag._replace(pix_to_face=frag.pix_to_face.long()), packed, d["opacity"], d["values"])


@pytest.mark.parametrize("K", (0, 33))
def test_k_out_of_range(K):
    d = _inputs(K=K)
    with pytest.raises(ValueError, match=rf"pack_slots_fused: K must be in 1\.\.32, got {K}"):
        FG.pack_slots_fused(d["frag"], d["F"])
    with pytest.raises(ValueError, match=rf"interpolate_packed_fused: K must be in 1\.\.32, got {K}"):
        FG.interpolate_packed_fused(d["frag"], d["packed"], d["faces"], d["attrs"])
    with pytest.raises(ValueError, match=rf"composite_values_packed_fused: K must be in 1\.\.32, got {K}"):
        FG.composite_values_packed_fused(d["frag"], d["packed"], d["opacity"], d["values"])


@pytest.mark.parametrize("Cn", (0, 257))
def test_c_out_of_range(Cn):
    d = _inputs(Cn=Cn)
    with pytest.raises(ValueError, match=rf"interpolate_packed_fused: C must be in 1\.\.256, got {Cn}"):
        FG.interpolate_packed_fused(d["frag"], d["packed"], d["faces"], d["attrs"])
    with pytest.raises(ValueError, match=rf"composite_values_packed_fused: C must be in 1\.\.256, got {Cn}"):
        FG.composite_values_packed_fused(d["frag"], d["packed"], d["opacity"], d["values"])


def test_shapes_and_arguments_that_do_not_match():
    d = _inputs()
    frag, packed, v = d["frag"], d["packed"], d["values"]
    with pytest.raises(ValueError, match=r"frag\.pix_to_face must be \[B,K,H,W\]"):
        FG.pack_slots_fused(frag._replace(pix_to_face=frag.pix_to_face[0]), d["F"])
    for bad in (-1, 2.0, True):
        with pytest.raises(ValueError, match="F must be a non-negative int"):
            FG.pack_slots_fused(frag, bad)
    with pytest.raises(ValueError, match=r"frag\.pix_to_face must be \[B,K,H,W\]"):
        FG.interpolate_packed_fused(frag._replace(pix_to_face=frag.pix_to_face[0]), packed, d["faces"], d["attrs"])
    with pytest.raises(ValueError, match=r"frag\.bary must be \[B,K,2,H,W\].*got None"):
        FG.interpolate_packed_fused(frag._replace(bary=None), packed, d["faces"], d["attrs"])
    with pytest.raises(ValueError, match=r"faces must be \[F,3\]"):
        FG.interpolate_packed_fused(frag, packed, d["faces"][:, :2], d["attrs"])
    with pytest.raises(ValueError, match=r"vert_attrs must be \[P,C\]"):
        FG.interpolate_packed_fused(frag, packed, d["faces"], d["attrs"][0])
    for bad in (packed.row[0], packed.row[:, :1], packed.row.permute(0, 1, 3, 2)):
        with pytest.raises(ValueError, match=r"packed\.row must have frag\.pix_to_face's shape"):
            FG.interpolate_packed_fused(frag, packed._replace(row=bad), d["faces"], d["attrs"])
        with pytest.raises(ValueError, match=r"packed\.row must have frag\.pix_to_face's shape"):
            FG.composite_values_packed_fused(frag, packed._replace(row=bad), d["opacity"], v)
    with pytest.raises(ValueError, match=r"packed\.n_used must hold one element"):
        FG.interpolate_packed_fused(frag, packed._replace(n_used=th.zeros(2, dtype=th.int32)), d["faces"], d["attrs"])
    with pytest.raises(ValueError, match=r"packed\.rows must be a non-negative int"):
        FG.interpolate_packed_fused(frag, packed._replace(rows=-1), d["faces"], d["attrs"])
    with pytest.raises(ValueError, match=r"faces_opacity must be \[F\]"):
        FG.composite_values_packed_fused(frag, packed, d["opacity"][:, None], v)
    for bad in (v[:-1], v[0], th.zeros(7, 3), v.t(), v[None]):
        with pytest.raises(ValueError, match=r"values must be \[packed\.rows, C\]"):
            FG.composite_values_packed_fused(frag, packed, d["opacity"], bad)
    for bad in (d["scale"][:, :-1], d["scale"][0], d["scale"].t()):
        with pytest.raises(ValueError, match=r"face_scale must be \[B,F\]"):
            FG.composite_values_packed_fused(frag, packed, d["opacity"], v, bad)


def test_a_binding_without_the_calls_says_rebuild(monkeypatch):
    """A `_C` of an older build (no SUPPORTS_FRAGMENT_PACKED, or False): a TypeError that says so, nothing is computed."""
    class Old:
        SUPPORTS_FRAGMENT_COMPOSITE = True
        SUPPORTS_FRAGMENT_TEXTURE = True
        SUPPORTS_FRAGMENT_VISIBILITY = True
        SUPPORTS_FRAGMENT_DEFERRED = True

    d = _inputs()
    monkeypatch.setattr(dmr, "_C", Old())
    with pytest.raises(TypeError, match=r"pack_slots_fused.*no fused fragment slot packing: rebuild.*" + PACK_PATH):
        FG.pack_slots_fused(d["frag"], d["F"])
    with pytest.raises(TypeError, match=r"interpolate_packed_fused.*no fused packed fragment interpolation: rebuild.*" + INTERP_PATH):
        FG.interpolate_packed_fused(d["frag"], d["packed"], d["faces"], d["attrs"])
    with pytest.raises(TypeError, match=r"composite_values_packed_fused.*no fused packed per-slot value compositing: rebuild.*" + VALUES_PATH):
        FG.composite_values_packed_fused(d["frag"], d["packed"], d["opacity"], d["values"])
    Old.SUPPORTS_FRAGMENT_PACKED = False
    with pytest.raises(TypeError, match="rebuild"):
        FG.pack_slots_fused(d["frag"], d["F"])


# ---------------------------------------------------------------------------
# Refusals of the C ABI, through ctypes with pointers that are never dereferenced (as tests/test_deferred_cpu.py): every check
# runs before any HIP call.  No call here has wholly valid arguments and an output to write: none reaches a launch.
# ---------------------------------------------------------------------------
D = C.c_void_p(16)  # non-null, never dereferenced on these paths
INT_MAX = 2 ** 31 - 1
CALLS = {
    "dmr_pack_slots": ("B K H W F capacity", "face row n_used stream"),
    "dmr_interpolate_packed": ("B K H W P F C N", "face bary row n_used faces vert_attrs out stream"),
    "dmr_interpolate_packed_backward": ("B K H W P F C N", "face bary row n_used faces vert_attrs grad_out dL_dvert_attrs dL_dbary stream"),
    "dmr_composite_values_packed": ("B K H W F C N", "face row faces_opacity values face_scale image T stream"),
    "dmr_composite_values_packed_backward": ("B K H W F C N", "face row n_used faces_opacity values face_scale grad_image grad_T "
                                             "dL_dfaces_opacity dL_dvalues dL_dface_scale stream"),
}
SIZES = dict(B=1, K=1, H=1, W=1, P=3, F=1, C=3, N=1, capacity=1)
NULL_BY_DEFAULT = ("face_scale", "stream", "dL_dvert_attrs", "dL_dbary", "dL_dfaces_opacity", "dL_dvalues", "dL_dface_scale")

# case -> (the arguments it changes, the text after "<call>: "; None: the call returns 0); a case that names an argument a call
# does not take is skipped for that call
EVERY_CALL = {
    "B=0": (dict(B=0), "bad dimensions"), "H=0": (dict(H=0), "bad dimensions"), "W=0": (dict(W=0), "bad dimensions"),
    "F<0": (dict(F=-1), "bad dimensions"), "P<0": (dict(P=-1), "bad dimensions"),
    "K=0": (dict(K=0), "K must be in 1..32, got 0"), "K=33": (dict(K=33), "K must be in 1..32, got 33"),
    "C=0": (dict(C=0), "C must be in 1..256, got 0"), "C=257": (dict(C=257), "C must be in 1..256, got 257"),
    "N<0": (dict(N=-1), "bad rows"), "capacity<0": (dict(capacity=-1), "bad rows"),
    "null face": (dict(face=None), "null fragment lists"), "null bary": (dict(bary=None), "null fragment lists"),
    "null faces": (dict(faces=None), "null faces"), "null vert_attrs": (dict(vert_attrs=None), "null vert_attrs"),
    "null faces_opacity": (dict(faces_opacity=None), "null faces_opacity"), "null values": (dict(values=None), "null values"),
    "tiles >= 2^31": (dict(B=INT_MAX, H=17, W=17), "problem too large"), "B K H W >= 2^31": (dict(K=32, H=65536, W=1024), "problem too large"),
    # two at once: the first check wins
    "bad K and bad rows": (dict(K=0, N=-1, capacity=-1), "K must be in 1..32, got 0"),
    "bad dimensions and bad K": (dict(W=0, K=99), "bad dimensions"),
    "bad rows and null lists": (dict(N=-1, capacity=-1, face=None), "bad rows"),
    "null lists and too large": (dict(face=None, K=32, H=65536, W=1024), "null fragment lists"),
}
PER_CALL = {
    "dmr_pack_slots": {"null row": (dict(row=None), "null output"), "null n_used": (dict(n_used=None), "null output"),
                       "too large and null output": (dict(K=32, H=65536, W=1024, row=None), "problem too large")},
    "dmr_interpolate_packed": {"null row": (dict(row=None), "null fragment lists"), "null n_used": (dict(n_used=None), "null n_used"),
                               "B F >= 2^31": (dict(B=65536, F=65536), "problem too large"),
                               "bad C and null lists": (dict(C=0, face=None), "C must be in 1..256, got 0"),
                               "null out": (dict(out=None), "null output"), "no rows, null out": (dict(N=0, out=None), None),
                               "null n_used and null out": (dict(n_used=None, out=None), "null n_used")},
    "dmr_interpolate_packed_backward": {"null row": (dict(row=None), "null fragment lists"), "null n_used": (dict(n_used=None), "null n_used"),
                                        "null grad_out": (dict(grad_out=None), "null grad_out"), "no gradient wanted": (dict(), None),
                                        "no rows, null grad_out, no gradient wanted": (dict(N=0, grad_out=None), None),
                                        "bad K although no gradient wanted": (dict(K=0), "K must be in 1..32, got 0")},
    "dmr_composite_values_packed": {"null row": (dict(row=None), "null fragment lists"), "null image": (dict(image=None), "null output"),
                                    "null T": (dict(T=None), "null output"), "B F >= 2^31": (dict(B=65536, F=65536), "problem too large"),
                                    "no rows, null values, null image": (dict(N=0, values=None, image=None), "null output"),
                                    "no faces, no opacities, null image": (dict(F=0, faces_opacity=None, image=None), "null output")},
    "dmr_composite_values_packed_backward": {"null row": (dict(row=None), "null fragment lists"), "null n_used": (dict(n_used=None), "null n_used"),
                                             "dL_dface_scale without face_scale": (dict(dL_dface_scale=D), "dL_dface_scale without face_scale"),
                                             "null n_used and dL_dface_scale without face_scale": (dict(n_used=None, dL_dface_scale=D), "null n_used"),
                                             "no gradient wanted": (dict(), None), "no gradient wanted, no upstream": (dict(grad_image=None, grad_T=None), None),
                                             "only dL_dvalues wanted, no rows": (dict(N=0, values=None, dL_dvalues=D), None),
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
            pair = case.startswith(("bad K and", "bad rows and"))   # (N or capacity: whichever the call takes)
            if all(k in takes for k in changes) or pair:
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
            assert ret == 1 and got == f"{call}: {text}", (call, case, got)
        seen.add((call, case))
    # every size check, the rows, the null lists, the null outputs and the pairs were tripped in every call they apply to
    for call in CALLS:
        for case in ("B=0", "H=0", "W=0", "F<0", "K=0", "K=33", "null face", "tiles >= 2^31", "B K H W >= 2^31", "bad K and bad rows",
                     "bad dimensions and bad K", "bad rows and null lists", "null lists and too large"):
            assert (call, case) in seen, (call, case)
        assert ((call, "N<0") in seen) != ((call, "capacity<0") in seen)
        assert ((call, "C=0") in seen and (call, "C=257") in seen) == (call != "dmr_pack_slots")
        assert all((call, case) in seen for case in PER_CALL[call])
    assert ("dmr_interpolate_packed", "P<0") in seen and ("dmr_interpolate_packed_backward", "null vert_attrs") in seen
    assert ("dmr_composite_values_packed", "null values") in seen and ("dmr_composite_values_packed", "P<0") not in seen


# ---------------------------------------------------------------------------
# The case tables of the GPU tests
# ---------------------------------------------------------------------------
def _all_cases():
    return [r for rows in PC.tables().values() for r in rows]


def test_dispatch_restated_as_the_unit_has_it():
    unit = UNIT_TEXT
    for line in PC.DISPATCH_LINES:
        assert unit.count(line) == 1 and COMMON_TEXT.count(line) == 0, line
    for line in PC.COMMON_DISPATCH_LINES:
        assert COMMON_TEXT.count(line) == 1 and unit.count(line) == 0, line
    assert '#include "%s"' % PC.COMMON_HEADER in unit
    assert [PC.interp_ch(c) for c in (1, 4, 5, 256)] == [4, 4, 8, 8]
    assert [PC.interp_via_lds(c) for c in (1, 4, 5, 8, 9, 32, 33, 256)] == [False, False, False, False, True, True, False, False]
    assert [PC.values_forward_ch(c) for c in (1, 4, 5, 256)] == [4, 4, 16, 16]
    assert [PC.values_backward_ch(c) for c in (1, 4, 5, 256)] == [4, 4, 8, 8]
    assert PC.PACK_SLOTS == 256 * 8 and [PC.pack_groups(n) for n in (1, 2047, 2048, 2049)] == [1, 1, 1, 2]
    # the kernels the unit instantiates are the ones every_instantiation lists
    named = set(re.findall(r"\b(k_[a-z_]+)<\w", unit)) - {"k_pack_count", "k_pack_scan", "k_pack_write"}   # (k_deferred_zero is the common header's)
    assert named == {k for k, _, _ in PC.every_instantiation()}


def test_the_unit_leaves_the_other_shading_units_alone():
    """No workgroup waits for another (the scan is three launches), and what is accumulated into is zeroed by a kernel of the
    unit (the common header's k_deferred_zero: the header's text is read along with the unit's)."""
    code = re.sub(r"//[^\n]*", "", COMMON_TEXT + UNIT_TEXT)
    assert "k_deferred_zero<<<" in code
    assert "hipMemsetAsync" not in code and "hipMalloc" not in code and "Synchronize" not in code
    assert "while (" not in code and "__builtin_amdgcn_s_sleep" not in code   # no spin on a flag
    assert all(k in code for k in ("k_pack_count<<<", "k_pack_scan<<<dim3(1)", "k_pack_write<<<"))


def test_tables_reach_every_instantiation():
    full = PC.every_instantiation()
    assert len(full) == 6 + 4 + 4 + 16
    reached = PC.instantiations(_all_cases())
    assert reached == full, sorted(full - reached, key=str)


def test_every_kmax_at_its_ends():
    ks = {r.K for r in _all_cases()}
    for kmax in PC.KMAXES:
        assert kmax in ks and PC.smallest_k(kmax) in ks, kmax
    cs = {r.C for r in _all_cases()}
    assert {1, 3, 4, 5, 35, 255, 256} <= cs and {8, 9, 32, 33} & cs != set() and any(PC.interp_via_lds(c) and c % 4 for c in cs)
    assert any(r.C == 4 and not r.aligned for r in _all_cases()) and any(r.C == 8 and not r.aligned for r in _all_cases())


def test_pack_shapes_meet_every_edge_of_the_scan():
    slots = [B * K * H * W for B, K, H, W in PC.PACK_SHAPES]
    assert 1 in slots and {PC.PACK_SLOTS - 1, PC.PACK_SLOTS, PC.PACK_SLOTS + 1} <= set(slots)
    groups = [PC.pack_groups(n) for n in slots]
    assert any(3 <= g <= PC.PACK_SCAN for g in groups) and any(g > PC.PACK_SCAN for g in groups)
