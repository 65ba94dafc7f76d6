"""The surface-frame unit without a GPU (csrc/dmr_surface.hip, include/dmesh_renderer_amd_surface.h, fragments.surface_packed /
surface_packed_fused): the header, the exports and the build lists; the C ABI's refusals in the order the header states, through
pointers that are never dereferenced; that the unit waits for nothing; the torch model's geometry in float64 (hit ==
interpolate_packed, unit normal towards the camera, the mirror, independence of the winding, a plane as a mirror), its degenerate
rules and its gradients (gradcheck); the fused entry point's refusals on CPU tensors; and the conditions on the inputs of
tests/test_surface_gpu.py's cases (surface_cases.py): the share of rows left out of the comparison of `normal`.
"""
import re

import pytest
import torch as th

import row_units as RU
import surface_cases as SC
from dmesh_renderer_amd import Fragments
from dmesh_renderer_amd import fragments as FG
from row_units import D

UNIT_TEXT, HEADER_TEXT = RU.unit_texts(SC.SOURCE, SC.HEADER)


# ---------------------------------------------------------------------------
# Library, binding and build lists
# ---------------------------------------------------------------------------
def test_library_exports_the_declared_symbols():
    RU.exports_declared(HEADER_TEXT, SC.FUNCTIONS)


def test_the_source_and_header_are_build_dependencies():
    RU.are_build_dependencies(SC.SOURCE, SC.HEADER, extra=["dmr_deferred_common.hpp", "dmr_shade_common.hpp"])


def test_binding_supports_it():
    from dmesh_renderer_amd import _C
    assert _C.SUPPORTS_FRAGMENT_SURFACE is True and callable(_C.surface_packed) and callable(_C.surface_packed_backward)
    assert {"SurfaceRows", "surface_packed", "surface_packed_fused"} <= set(FG.__all__) and FG.SurfaceRows._fields == SC.OUTPUTS
    assert "surface_packed_fused makes that direction" in FG.__doc__


def test_the_unit_waits_for_nothing_and_zeroes_nothing_by_memset():
    code = RU.waits_for_nothing([UNIT_TEXT], fill_calls=2, extra_forbidden=["zero_on("])   # (dL_dverts and dL_dorigin)
    # every check precedes every launch: in both calls nothing is enqueued before the last refusal
    for call in SC.FUNCTIONS:
        body = code[code.index(f"int {call}("):]
        body = body[:body.index("\n}\n")]
        enqueues = [body.index(w) for w in ("<<<", "rows_fill_on(", "launch_surface_backward<") if w in body]
        assert enqueues and max(body.rindex("api_fail("), body.index("surface_params(")) < min(enqueues), call


def test_the_product_launches_every_instantiation_once():
    launches = re.findall(r"launch_surface_backward<(true|false), (true|false), (true|false)>\(p, st", UNIT_TEXT)
    got = {("k_surface_packed_backward", tuple(x == "true" for x in l)) for l in launches}
    assert len(launches) == 7 and got | {("k_surface_packed", ())} == SC.every_instantiation()
    assert UNIT_TEXT.count("k_surface_packed<<<") == 1 and "DMR_ABLATION" not in UNIT_TEXT
    for g in (("verts",), ("bary",), ("origin", "verts"), SC.GRADS):
        assert SC.instantiation(g) in SC.every_instantiation()
    assert SC.instantiation(()) is None


# ---------------------------------------------------------------------------
# The C ABI's refusals
# ---------------------------------------------------------------------------
SIZES = dict(B=1, K=1, H=2, W=2, P=3, F=1, N=1)
NULL_BY_DEFAULT = ("dL_dverts", "dL_dbary", "dL_dorigin")
HUGE = dict(B=2, K=32, H=8192, W=8192)
NO_UPSTREAM = dict(grad_hit=None, grad_normal=None, grad_reflect=None)
EVERY_CALL = {
    "B=0": (dict(B=0), "bad dimensions"), "H<0": (dict(H=-1), "bad dimensions"), "W=0": (dict(W=0), "bad dimensions"),
    "P<0": (dict(P=-1), "bad dimensions"), "F<0": (dict(F=-2), "bad dimensions"),
    "K=0": (dict(K=0), "K must be in 1..32, got 0"), "K=33": (dict(K=33), "K must be in 1..32, got 33"),
    "N<0": (dict(N=-1), "bad rows"),
    "null face": (dict(face=None), "null fragment lists"), "null bary": (dict(bary=None), "null fragment lists"),
    "null row": (dict(row=None), "null fragment lists"),
    "null faces": (dict(faces=None), "null faces"),
    "null verts": (dict(verts=None), "null verts / origin"), "null origin": (dict(origin=None), "null verts / origin"),
    "null origin without faces": (dict(origin=None, F=0, faces=None, verts=None), "null verts / origin"),
    "null n_used": (dict(n_used=None), "null n_used"),
    "too large": (HUGE, "problem too large"),
    # two at once: the first check in the header's order wins
    "bad dimensions and bad K": (dict(B=-1, K=0), "bad dimensions"), "bad K and bad rows": (dict(K=40, N=-1), "K must be in 1..32, got 40"),
    "bad rows and null lists": (dict(N=-5, face=None), "bad rows"), "null lists and null faces": (dict(row=None, faces=None), "null fragment lists"),
    "null faces and null verts": (dict(faces=None, verts=None), "null faces"), "null verts and null n_used": (dict(verts=None, n_used=None), "null verts / origin"),
    "null n_used and too large": (dict(HUGE, n_used=None), "null n_used"),
}
PER_CALL = {
    "dmr_surface_packed": {
        "null hit": (dict(hit=None), "null output"), "null normal": (dict(normal=None), "null output"), "null reflect": (dict(reflect=None), "null output"),
        "too large and a null output": (dict(HUGE, hit=None), "problem too large"),
        "no rows": (dict(N=0), None), "no rows, null outputs": (dict(N=0, hit=None, normal=None, reflect=None), None),
        "no rows but null n_used": (dict(N=0, n_used=None), "null n_used")},
    "dmr_surface_packed_backward": {
        "no gradient wanted": (dict(), None),
        "no upstream": (dict(NO_UPSTREAM, dL_dbary=D), "null upstreams"), "no upstream, no gradient wanted": (NO_UPSTREAM, "null upstreams"),
        "too large and no upstream": (dict(HUGE, **NO_UPSTREAM), "problem too large"),
        "no rows, no upstream, no gradient wanted": (dict(NO_UPSTREAM, N=0), None),
        "bad K although no gradient wanted": (dict(K=64), "K must be in 1..32, got 64")},
}


def test_c_abi_refusals():
    import capi_ctypes
    lib = SC.declare(capi_ctypes.load())
    RU.run_refusals(lib, SC.INTS, SC.PTRS, SIZES, NULL_BY_DEFAULT, EVERY_CALL, PER_CALL)
    # the order the header documents is the order tested above
    order = re.sub(r"\s*\n \* ", " ", HEADER_TEXT[HEADER_TEXT.index("The first check that fails"):])
    at = [order.index(w) for w in ("the sizes (B, H, W, P, F; K)", '"bad rows"', "null lists", "null faces", "null verts / origin", "null n_used",
                                   '"problem too large"', "a null output", "all three upstreams null", "no gradient wanted")]
    assert at == sorted(at) and "Every check precedes every launch" in order


# ---------------------------------------------------------------------------
# The model in float64
# ---------------------------------------------------------------------------
def _f64(c, leaves=()):
    d = SC.lists(c)
    t = {k: d[k].double() for k in ("bary", "verts", "origin")}
    for k in leaves:
        t[k].requires_grad_(True)
    return d, t, FG.surface_packed(Fragments(d["face"], t["bary"], None), d["packed"], d["faces"], t["verts"], t["origin"])


def _directions(d, t, s):
    """d of every held row, from the model's own hit points and the slots' views."""
    B = d["face"].shape[0]
    view = th.zeros(d["packed"].rows, dtype=th.long)
    live = d["packed"].row >= 0
    view[d["packed"].row[live].long()] = th.arange(B).view(B, 1, 1, 1).expand_as(live)[live]
    w = s.hit.detach() - t["origin"].detach()[view]
    return w / w.norm(dim=1, keepdim=True)


@pytest.mark.parametrize("c", [SC.TABLE[1], SC.TABLE[5], SC.TABLE[3], SC.OTHER_F, SC.CAPACITY[0], SC.CAPACITY[2]], ids=str)
def test_model_geometry(c):
    d, t, s = _f64(c)
    held = d["held"]
    assert all(tuple(x.shape) == (d["packed"].rows, 3) and x.dtype == th.float64 for x in s) and int(held.sum()) > 0
    assert th.equal(s.hit, FG.interpolate_packed(Fragments(d["face"], t["bary"], None), d["packed"], d["faces"], t["verts"]))
    dirs = _directions(d, t, s)[held]
    n, r = s.normal[held], s.reflect[held]
    assert float((n.norm(dim=1) - 1).abs().max()) <= 1e-12 and float((r.norm(dim=1) - 1).abs().max()) <= 1e-12
    assert float((n * dirs).sum(1).max()) <= 1e-12
    assert float((r - (dirs - 2 * (dirs * n).sum(1, keepdim=True) * n)).abs().max()) <= 1e-12
    for x in s:   # every row no counting slot holds is 0
        assert float(x[~held].abs().sum()) == 0.0
    # neither output knows the winding of a face
    swapped = FG.surface_packed(Fragments(d["face"], t["bary"][:, :, [1, 0]], None), d["packed"], d["faces"][:, [0, 2, 1]], t["verts"], t["origin"])
    assert float((swapped.hit - s.hit).abs().max()) <= 1e-12
    assert float((swapped.normal - s.normal).abs().max()) <= 1e-12 and float((swapped.reflect - s.reflect).abs().max()) <= 1e-12


def test_a_plane_is_a_mirror():
    """The plane z = 0 seen from (0, 0, 1): (dx, dy, dz) leaves as (dx, dy, -dz), the normal is +z whatever the winding."""
    verts = th.tensor([[-4.0, -4, 0], [4, -4, 0], [4, 4, 0], [-4, 4, 0]], dtype=th.float64)
    faces = th.tensor([[0, 1, 2], [0, 3, 2]], dtype=th.int32)   # (opposite windings)
    g = th.Generator().manual_seed(1)
    face = th.randint(0, 2, (1, 3, 5, 7), generator=g, dtype=th.int32)
    bu = th.rand(1, 3, 1, 5, 7, generator=g, dtype=th.float64)
    bary = th.cat([bu, (1 - bu) * th.rand(1, 3, 1, 5, 7, generator=g, dtype=th.float64)], 2)
    frag = Fragments(face, bary, None)
    packed = FG.pack_slots(frag, 2)
    origin = th.tensor([[0.0, 0, 1]], dtype=th.float64)
    s = FG.surface_packed(frag, packed, faces, verts, origin)
    d = (s.hit - origin) / (s.hit - origin).norm(dim=1, keepdim=True)
    assert packed.rows == 105 and float(s.hit[:, 2].abs().max()) == 0.0
    assert float((s.reflect - d * th.tensor([1.0, 1, -1], dtype=th.float64)).abs().max()) <= 1e-12
    assert float((s.normal - th.tensor([0.0, 0, 1], dtype=th.float64)).abs().max()) <= 1e-12


def test_degenerate_faces():
    """Two equal vertices, and three collinear ones: normal 0, reflect the view direction, nothing into verts through the normal."""
    d, t, s = _f64(SC.DEGENERATE, leaves=("verts", "bary", "origin"))
    flat = th.isin(d["face"], th.tensor([1, 2], dtype=th.int32)) & (d["packed"].row >= 0)
    rows = d["packed"].row[flat].long()
    assert len(rows) > 100
    dirs = _directions(d, t, s)
    assert float(s.normal[rows].detach().abs().max()) == 0.0 and float((s.reflect[rows].detach() - dirs[rows]).abs().max()) <= 1e-12
    assert float(s.normal.detach()[d["held"]].norm(dim=1).min()) == 0.0 and float(s.normal.detach().norm(dim=1).max()) <= 1 + 1e-12
    up = th.zeros_like(s.normal)
    up[rows] = 1.0
    gv, gb, go = th.autograd.grad((s.normal * up).sum(), [t["verts"], t["bary"], t["origin"]], retain_graph=True, allow_unused=True)
    assert float(gv.abs().max()) == 0.0 and gb is None and go is None   # (the sign is a constant: the normal knows neither (u, v) nor the camera)
    grads = th.autograd.grad((s.hit * up).sum() + (s.reflect * up).sum() + s.normal.sum(), [t["verts"], t["bary"], t["origin"]])
    assert all(bool(th.isfinite(x).all()) and float(x.abs().max()) > 0 for x in grads)


def test_a_hit_at_the_camera_centre():
    d, t, s = _f64(SC.AT_ORIGIN, leaves=("verts", "bary", "origin"))
    r = int(d["packed"].row[0, 0, 0, 0])
    assert r >= 0 and th.equal(s.hit[r].detach(), t["origin"][0].detach()) and float(s.reflect[r].detach().abs().max()) == 0.0 and abs(float(s.normal[r].detach().norm()) - 1) <= 1e-12
    up = th.zeros_like(s.hit)
    up[r] = 1.0
    for out in (s.reflect, s.normal):
        grads = th.autograd.grad((out * up).sum(), [t["verts"], t["bary"], t["origin"]], retain_graph=True, allow_unused=True)
        assert all(x is None or bool(th.isfinite(x).all()) for x in grads) and (grads[2] is None or float(grads[2].abs().max()) == 0.0)
    grads = th.autograd.grad(sum((x * th.nan_to_num(d[k]).double()).sum() for x, k in zip(s, SC.UPSTREAMS)), [t["verts"], t["bary"], t["origin"]])
    assert all(bool(th.isfinite(x).all()) and float(x.abs().max()) > 0 for x in grads)


def test_model_gradients():
    """gradcheck of all three outputs in verts, bary and origin on a case with no row within 1e-2 of s = 0."""
    g = th.Generator().manual_seed(4)
    verts = th.rand(6, 3, generator=g, dtype=th.float64)
    faces = th.tensor([[0, 1, 2], [3, 2, 1], [4, 5, 0], [2, 5, 3]], dtype=th.int32)
    face = th.randint(-1, 6, (2, 2, 2, 3), generator=g, dtype=th.int32)   # (-1: empty; 4, 5: past F)
    bary = th.rand(2, 2, 2, 2, 3, generator=g, dtype=th.float64) * 0.4 + 0.05
    origin = th.tensor([[0.4, 0.6, 3.0], [3.0, -2.0, 0.5]], dtype=th.float64)
    frag = Fragments(face, bary, None)
    packed = FG.pack_slots(frag, 4, 20)
    s = FG.surface_packed(frag, packed, faces, verts, origin)
    d = th.nn.functional.normalize(s.reflect - 2 * (s.reflect * s.normal).sum(1, keepdim=True) * s.normal, dim=1)
    used = s.normal.norm(dim=1) > 0
    assert 8 <= int(used.sum()) < 20 and float((s.normal * d).sum(1)[used].abs().min()) > 1e-2

    def f(v, b, o):
        return tuple(FG.surface_packed(Fragments(face, b, None), packed, faces, v, o))

    assert th.autograd.gradcheck(f, (verts.requires_grad_(True), bary.requires_grad_(True), origin.requires_grad_(True)), eps=1e-6, atol=1e-7)


# ---------------------------------------------------------------------------
# The fused entry point's refusals (no kernel is reached on CPU tensors)
# ---------------------------------------------------------------------------
def test_fused_refusals_on_cpu_tensors():
    d = SC.lists(SC.TABLE[0])
    frag, packed = Fragments(d["face"], d["bary"], None), d["packed"]
    good = dict(frag=frag, packed=packed, faces=d["faces"], verts=d["verts"], origin=d["origin"])
    for change, what in ((dict(), "frag.pix_to_face is on cpu"), (dict(verts=d["verts"].double()), "verts must be float32"),
                         (dict(origin=d["origin"].half()), "origin must be float32"), (dict(faces=d["faces"].float()), "faces must be an integer tensor"),
                         (dict(frag=Fragments(d["face"].long(), d["bary"], None)), "frag.pix_to_face must be int32"),
                         (dict(packed=packed._replace(row=packed.row.long())), "packed.row must be int32")):
        with pytest.raises(TypeError, match=r"surface_packed_fused: .*fragments\.surface_packed is the torch path") as e:
            FG.surface_packed_fused(**dict(good, **change))
        assert what in str(e.value), (what, str(e.value))
    for fn in (FG.surface_packed, FG.surface_packed_fused):
        for change, what in ((dict(origin=d["origin"][0]), r"origin must be \[B,3\] = \(1, 3\)"), (dict(origin=th.zeros(2, 3)), r"origin must be \[B,3\]"),
                             (dict(origin=th.zeros(1, 4)), r"origin must be \[B,3\]"), (dict(verts=th.zeros(9, 4)), r"verts must be \[P,3\]"),
                             (dict(faces=d["faces"][:, :2]), r"faces must be \[F,3\]"), (dict(frag=Fragments(d["face"], None, None)), "frag.bary must be"),
                             (dict(packed=packed._replace(row=packed.row[:, :, :5])), "packed.row must have frag.pix_to_face's shape"),
                             (dict(packed=packed._replace(rows=-1)), "packed.rows must be a non-negative int")):
            with pytest.raises(ValueError, match=fn.__name__ + ": " + what):
                fn(**dict(good, **change))


# ---------------------------------------------------------------------------
# The GPU tests' inputs
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("c", list(dict.fromkeys(SC.all_cases())), ids=str)
def test_case_inputs(c):
    """At most NEAR_SHARE of a case's held rows lie within NEAR of s = 0 (they are left out of the comparison of `normal`), no
    face is thin unless it is meant to be, the origins of the plain cases are 2 to 4 from the box's middle, and the upstreams are
    NaN exactly in the rows no counting slot holds."""
    d = SC.lists(c)
    held, near = d["held"], d["near"]
    assert int(held.sum()) > 0 and int(near.sum()) <= SC.NEAR_SHARE * int(held.sum())
    if c.special is None:
        assert 2 <= float((d["origin"] - 0.5).norm(dim=1).min()) and float((d["origin"] - 0.5).norm(dim=1).max()) <= 4
        assert float(SC._areas(d["faces"], d["verts"]).min()) >= SC.MIN_AREA
    for k in SC.UPSTREAMS:
        assert th.equal(th.isnan(d[k]).any(1), ~held) and th.equal(th.isnan(d[k]).all(1), ~held)
    assert float(d["grad_normal"][near].abs().sum()) == 0.0
    N, count = d["packed"].rows, d["count"]
    assert {None: N == count, -300: N < count, 0: N == count, 130: N > count}[c.cap] and (c.extra_f == 0 or int(held.sum()) < count)
    assert float(d["verts"].min()) >= 0 and float(d["verts"].max()) <= 1
