"""fragments.interpolate_fused and fragments.composite_values_fused on the GPU (csrc/dmr_interp.hip: k_interpolate_fragments,
k_interpolate_fragments_backward, k_composite_values, k_composite_values_backward) against fragments.interpolate and
fragments.composite_values evaluated in float64 on the CPU, on the same float32 inputs cast up, ids past F set to -1 for the model.

Bounds (the project's own): forward rel_err <= FWD_TOL = 1e-5, gradients rel_err <= GRAD_TOL = 1e-4 (scenes.rel_err); two
evaluations of the same sums in another order <= sum_order_tol(name).  Every case prints what it measured (pytest -s).

MEASURED on the MI355X, the largest figure over all 117 cases (rel_err against the float64 models): interpolate_fused out 1.8e-7,
dL_dvert_attrs 2.4e-7, dL_dbary 2.0e-7; composite_values_fused image 2.0e-7, T 2.0e-7, dL_dfaces_opacity 2.9e-7, dL_dvalues
1.7e-7, dL_dface_scale 3.1e-7.  The misaligned calls give the aligned calls' forward bit for bit, dL_dvert_attrs to 1.3e-7,
dL_dbary equal.  The chain against composite_fused: image and T equal bit for bit, gradients to 1.8e-7 (bary).  A NaN / an Inf in
every empty slot: every output and gradient bit-equal to the run without.  Rendered lists: colour to 8.9e-8 (tri), 6.0e-8 (tet);
verts.grad against the torch path 6.8e-7 (tri, max |ref| 14.1), 1.3e-7 (tet, max |ref| 114).  Graph replays against eager: the
stored outputs (image, T, bary) equal, the accumulated ones to 8.6e-8, and exactly 0 where no tile wrote.
"""
import functools

import numpy as np
import pytest
import torch as th

import deferred_cases as DC
from dmesh_renderer_amd import Fragments, scenes
from dmesh_renderer_amd import fragments as FG
from harness import TET_ARGS, TRI_ARGS, capture_replay, replay
from shading_cases import EDGE_FRAMES, FRAME, MERGE_F, MERGE_FRAME, MERGE_K, MERGE_P, NEW_FRAME, SIZES, one_float_in
from util import rel_err, sum_order_tol

pytestmark = pytest.mark.gpu

FWD_TOL = 1e-5
GRAD_TOL = 1e-4
INT32_MAX = 2 ** 31 - 1
GRADS_I = ("vert_attrs", "bary")                       # interpolate_fused
GRADS_V = ("faces_opacity", "values", "face_scale")    # composite_values_fused


@functools.lru_cache(maxsize=None)
def _lists(K, C, size, frame=FRAME):
    """Caller-made lists (CPU float32 / int32), as test_composite_fused_gpu._lists makes them: 15 % of the slots -1, 10 % ids
    past F, anywhere in a list; one face of opacity exactly 1 and one of opacity exactly 0, the others small enough that T_K
    is not 0 at K = 32; per-slot values, and signed upstreams of out, image and T."""
    B, H, W = frame
    F, P = SIZES[size]
    g = th.Generator().manual_seed(3000 * K + 10 * C + (F > 100) + 7 * H)
    face = th.randint(0, F, (B, K, H, W), generator=g, dtype=th.int32)
    r = th.rand(B, K, H, W, generator=g)
    face = th.where(r < 0.15, th.full_like(face, -1), face)
    face = th.where((r >= 0.15) & (r < 0.25), face + F + (face % 3) * 5, face)  # F, F + 5.., past the faces
    bary = th.rand(B, K, 2, H, W, generator=g) * 0.6 - 0.05
    faces = th.randint(0, P, (F, 3), generator=g, dtype=th.int32)
    opacity = th.rand(F, generator=g) * (0.12 if K > 5 else 0.6) + 0.01
    opacity[1], opacity[4] = 1.0, 0.0
    return dict(face=face, bary=bary, faces=faces, faces_opacity=opacity, vert_attrs=th.randn(P, C, generator=g),
                face_scale=th.rand(B, F, generator=g) + 0.5, values=th.randn(B, K, C, H, W, generator=g),
                g_out=th.randn(B, K, C, H, W, generator=g), g_image=th.randn(B, C, H, W, generator=g), g_T=th.randn(B, 1, H, W, generator=g))


def _model_face(d):
    F = d["faces_opacity"].shape[0]
    return th.where(d["face"] >= F, th.full_like(d["face"], -1), d["face"])


def _interp_model(d):
    """fragments.interpolate in float64 on the CPU -> out, {name: grad} (numpy)."""
    lv = {k: d[k].double().requires_grad_(True) for k in GRADS_I}
    out = FG.interpolate(Fragments(_model_face(d), lv["bary"], None), d["faces"], lv["vert_attrs"])
    (out * d["g_out"].double()).sum().backward()
    return out.detach().numpy(), {k: v.grad.numpy() for k, v in lv.items()}


def _values_model(d, with_scale):
    """fragments.composite_values in float64 on the CPU -> image, T, {name: grad} (numpy)."""
    lv = {k: d[k].double().requires_grad_(True) for k in GRADS_V if with_scale or k != "face_scale"}
    image, T = FG.composite_values(Fragments(_model_face(d), None, None), lv["faces_opacity"], lv["values"], lv.get("face_scale"))
    ((image * d["g_image"].double()).sum() + (T * d["g_T"].double()).sum()).backward()
    return image.detach().numpy(), T.detach().numpy(), {k: v.grad.numpy() for k, v in lv.items()}


@functools.lru_cache(maxsize=None)
def _interp_reference(K, C, size, frame=FRAME):
    return _interp_model(_lists(K, C, size, frame))


@functools.lru_cache(maxsize=None)
def _values_reference(K, C, size, with_scale, frame=FRAME):
    return _values_model(_lists(K, C, size, frame), with_scale)


def _interp_fused(d, dev, want=GRADS_I, leaves=None):
    """interpolate_fused on the device, gradients of `want` only -> out, {name: grad}.  leaves: {name: the device tensor to
    differentiate, as it is (its storage and offset)} in place of a fresh copy of d[name]."""
    t = {k: d[k].to(dev) for k in ("face", "bary", "faces", "vert_attrs", "g_out")}
    lv = {k: (leaves[k].detach() if leaves and k in leaves else t[k].clone()).requires_grad_(True) for k in want}
    out = FG.interpolate_fused(Fragments(t["face"], lv.get("bary", t["bary"]), None), t["faces"], lv.get("vert_attrs", t["vert_attrs"]))
    grads = th.autograd.grad((out * t["g_out"]).sum(), [lv[k] for k in want]) if want else ()
    return out.detach(), dict(zip(want, grads))


def _values_fused(d, dev, with_scale, want=GRADS_V, g_image=True, g_T=True):
    """composite_values_fused on the device, gradients of `want` only -> image, T, {name: grad}."""
    t = {k: d[k].to(dev) for k in ("face", "faces_opacity", "values", "face_scale", "g_image", "g_T")}
    names = [k for k in want if with_scale or k != "face_scale"]
    lv = {k: t[k].clone().requires_grad_(True) for k in names}
    image, T = FG.composite_values_fused(Fragments(t["face"], None, None), lv.get("faces_opacity", t["faces_opacity"]), lv.get("values", t["values"]),
                                         lv.get("face_scale", t["face_scale"]) if with_scale else None)
    loss = 0
    if g_image:
        loss = loss + (image * t["g_image"]).sum()
    if g_T:
        loss = loss + (T * t["g_T"]).sum()
    grads = th.autograd.grad(loss, [lv[k] for k in names]) if names else ()
    return image.detach(), T.detach(), dict(zip(names, grads))


def check_inputs(refs):
    """What a case's inputs must give before anything is compared: a non-zero float64 reference for every tensor (an all-empty
    list cannot pass).  refs: {name: numpy}."""
    for k, r in refs.items():
        assert float(np.abs(r).max()) > 0, k


def _empty(d):
    F = d["faces_opacity"].shape[0]
    return (d["face"] < 0) | (d["face"] >= F)


def _check_interp(tag, d, ref, got):
    out_r, g_r = ref
    out, g = got
    check_inputs(dict(g_r, out=out_r))
    assert tuple(out.shape) == out_r.shape and out.dtype == th.float32
    e = rel_err(out.cpu().numpy(), out_r)
    print(f"\n{tag}: interpolate out {e:.2e} (max |out| {np.abs(out_r).max():.3g})")
    assert e <= FWD_TOL
    assert set(g) == set(g_r)
    for k, r in g_r.items():
        x = g[k].cpu().numpy()
        assert x.shape == r.shape and x.dtype == np.float32
        eg = rel_err(x, r)
        print(f"  dL_d{k} {eg:.2e} (max |ref| {np.abs(r).max():.3g})")
        assert eg <= GRAD_TOL, (k, eg)
    empty = _empty(d)
    if bool(empty.any()):  # exact zeros in the empty slots of out and of dL/dbary
        assert float(out.cpu()[empty[:, :, None].expand_as(out)].abs().max()) == 0.0
        assert float(g["bary"].cpu()[empty[:, :, None].expand(-1, -1, 2, -1, -1)].abs().max()) == 0.0


def _check_values(tag, d, ref, got):
    image_r, T_r, g_r = ref
    image, T, g = got
    check_inputs(dict(g_r, image=image_r, T=T_r))
    assert tuple(image.shape) == image_r.shape and tuple(T.shape) == T_r.shape and image.dtype == T.dtype == th.float32
    ei, eT = rel_err(image.cpu().numpy(), image_r), rel_err(T.cpu().numpy(), T_r)
    print(f"\n{tag}: composite_values image {ei:.2e} T {eT:.2e} (max |image| {np.abs(image_r).max():.3g})")
    assert ei <= FWD_TOL and eT <= FWD_TOL
    assert set(g) == set(g_r)
    for k, r in g_r.items():
        x = g[k].cpu().numpy()
        assert x.shape == r.shape and x.dtype == np.float32
        eg = rel_err(x, r)
        print(f"  dL_d{k} {eg:.2e} (max |ref| {np.abs(r).max():.3g})")
        assert eg <= GRAD_TOL, (k, eg)
    empty = _empty(d)
    if bool(empty.any()):  # exact zeros in dL/dvalues
        assert float(g["values"].cpu()[empty[:, :, None].expand_as(g["values"])].abs().max()) == 0.0


@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("C", DC.LISTS_C)
@pytest.mark.parametrize("K", DC.LISTS_K)
def test_caller_made_lists_interpolate(hip_device, K, C, size):
    """(1) out and the gradients of vert_attrs and bary against the float64 model: P = 9 (every lane of a wave merges) and
    P = 9000 (a tile holds more vertex rows than the table's 560 slots: rows leave with direct atomics), partial tiles in both
    axes.  (What the MI355X run printed: MEASURED, at the top.)"""
    d = _lists(K, C, size)
    _check_interp(f"K {K} C {C} {size}", d, _interp_reference(K, C, size), _interp_fused(d, hip_device))


@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("with_scale", (False, True), ids=("no_scale", "scale"))
@pytest.mark.parametrize("C", DC.LISTS_C)
@pytest.mark.parametrize("K", DC.LISTS_K)
def test_caller_made_lists_composite_values(hip_device, K, C, with_scale, size):
    """(1) image, T and the gradients of faces_opacity, values and face_scale against the float64 model: F = 7 and F = 6000."""
    d = _lists(K, C, size)
    _check_values(f"K {K} C {C} {size} scale {with_scale}", d, _values_reference(K, C, size, with_scale), _values_fused(d, hip_device, with_scale))


@pytest.mark.parametrize("K,C,size", DC.MATRIX, ids=[f"K{K}-C{C}-{size}" for K, C, size in DC.MATRIX])
def test_instantiation_matrix(hip_device, K, C, size):
    """(2) every KMAX of the blend's backward at K == KMAX and at the first K of the next, against the channel chunks (float4 rows
    at C = 4, one CH 8 walk, one CH 16 walk, a cut one at C = 20, scalar C = 3), DEFER_MAX_C and the scalar below it, on a 17 x 33
    view: both pairs against their float64 models.  Where C % 4 == 0, interpolate_fused again with vert_attrs one float off a
    16-byte boundary (scalar loads): forward bit-equal to the aligned call, gradients within sum_order_tol."""
    dev = hip_device
    d = _lists(K, C, size, NEW_FRAME)
    ref = _interp_reference(K, C, size, NEW_FRAME)
    own = d["vert_attrs"].to(dev).clone()
    assert own.data_ptr() % 16 == 0
    alg = _interp_fused(d, dev, leaves={"vert_attrs": own})
    _check_interp(f"K {K} C {C} {size}", d, ref, alg)
    _check_values(f"K {K} C {C} {size}", d, _values_reference(K, C, size, True, NEW_FRAME), _values_fused(d, dev, True))
    if C % 4 == 0:
        off = one_float_in(d["vert_attrs"].to(dev))
        assert off.is_contiguous() and off.data_ptr() % 16 == 4 and bool((off == own).all())
        got = _interp_fused(d, dev, leaves={"vert_attrs": off})
        _check_interp(f"K {K} C {C} {size} misaligned", d, ref, got)
        print(f"misaligned vs aligned: forward bit-equal: {bool(th.equal(got[0], alg[0]))}")
        assert th.equal(got[0], alg[0])
        for k in GRADS_I:
            e = rel_err(got[1][k].cpu().numpy(), alg[1][k].cpu().numpy())
            print(f"  dL_d{k} misaligned vs aligned {e:.2e}")
            assert e <= sum_order_tol(k), (k, e)


def _chain(t, lv, with_scale=True):
    """composite_values_fused(interpolate_fused(...)) on device tensors -> image, T."""
    a = FG.interpolate_fused(Fragments(t["face"], lv.get("bary", t["bary"]), None), t["faces"], lv.get("vert_attrs", t["vert_attrs"]))
    return FG.composite_values_fused(Fragments(t["face"], None, None), lv.get("faces_opacity", t["faces_opacity"]), a,
                                     lv.get("face_scale", t["face_scale"]) if with_scale else None)


CHAIN_GRADS = ("faces_opacity", "vert_attrs", "face_scale", "bary")


@pytest.mark.parametrize("K,C,size", DC.IDENTITY, ids=[f"K{K}-C{C}-{size}" for K, C, size in DC.IDENTITY])
def test_identity_on_the_device(hip_device, K, C, size):
    """(3) composite_values_fused(frag, o, interpolate_fused(frag, faces, A), s) against composite_fused(frag, faces, o, A, s) on
    the same lists: image and T within FWD_TOL, the gradients of o, A, s and bary through the chain within GRAD_TOL of
    composite_fused's."""
    dev = hip_device
    d = _lists(K, C, size)
    t = {k: v.to(dev) for k, v in d.items()}
    res = []
    for fn in (_chain, lambda t, lv: FG.composite_fused(Fragments(t["face"], lv["bary"], None), t["faces"], lv["faces_opacity"],
                                                         lv["vert_attrs"], face_scale=lv["face_scale"])):
        lv = {k: t[k].clone().requires_grad_(True) for k in CHAIN_GRADS}
        image, T = fn(t, lv)
        grads = th.autograd.grad((image * t["g_image"]).sum() + (T * t["g_T"]).sum(), [lv[k] for k in CHAIN_GRADS])
        res.append((image.detach().cpu().numpy(), T.detach().cpu().numpy(), [g.cpu().numpy() for g in grads]))
    (ia, Ta, ga), (ib, Tb, gb) = res
    ei, eT = rel_err(ia, ib), rel_err(Ta, Tb)
    print(f"\nK {K} C {C} {size}: chain vs composite_fused image {ei:.2e} T {eT:.2e} (max |image| {np.abs(ib).max():.3g})")
    assert float(np.abs(ib).max()) > 0 and ei <= FWD_TOL and eT <= FWD_TOL
    for k, a, b in zip(CHAIN_GRADS, ga, gb):
        e = rel_err(a, b)
        print(f"  dL_d{k} {e:.2e} (max |composite_fused's| {np.abs(b).max():.3g})")
        assert float(np.abs(b).max()) > 0 and e <= GRAD_TOL, (k, e)


def test_only_some_gradients_wanted(hip_device):
    """(4) each output gradient alone equals all of them together, and none at all; grad_image alone and grad_T alone add up to
    the model's gradients; unwanted ones come back None."""
    from dmesh_renderer_amd import _C
    dev = hip_device
    K, C, size = DC.ONLY_SOME
    d = _lists(K, C, size)
    _, g_all = _interp_fused(d, dev)
    for k in GRADS_I:
        _, g = _interp_fused(d, dev, want=(k,))
        e = rel_err(g[k].cpu().numpy(), g_all[k].cpu().numpy())
        print(f"\ninterpolate dL_d{k} alone vs both: {e:.2e}")
        assert list(g) == [k] and e <= sum_order_tol(k), (k, e)
    out, g = _interp_fused(d, dev, want=())
    assert g == {} and not out.requires_grad
    _, _, v_all = _values_fused(d, dev, True)
    for k in GRADS_V:
        _, _, g = _values_fused(d, dev, True, want=(k,))
        e = rel_err(g[k].cpu().numpy(), v_all[k].cpu().numpy())
        print(f"composite_values dL_d{k} alone vs all three: {e:.2e}")
        assert list(g) == [k] and e <= sum_order_tol(k), (k, e)
    _, _, g_T = _values_fused(d, dev, True, g_image=False)
    _, _, g_I = _values_fused(d, dev, True, g_T=False)
    _, _, ref = _values_reference(K, C, size, True)
    for k in GRADS_V:
        e = rel_err((g_T[k] + g_I[k]).cpu().numpy(), ref[k])
        print(f"dL_d{k}: only grad_T + only grad_image vs the model {e:.2e}")
        assert e <= GRAD_TOL, (k, e)
    for k in ("values", "face_scale"):  # T depends on the opacities alone
        assert float(g_T[k].abs().max()) == 0.0, k
    t = {k: v.to(dev) for k, v in d.items()}
    assert _C.interpolate_fragments_backward(t["face"], t["bary"], t["faces"], t["vert_attrs"], t["g_out"], (False, False)) == (None, None)
    assert _C.composite_values_backward(t["face"], t["faces_opacity"], t["values"], t["face_scale"], t["g_image"], t["g_T"],
                                        (False, False, False)) == (None, None, None)
    got = _C.composite_values_backward(t["face"], t["faces_opacity"], t["values"], None, t["g_image"], None, (False, True, False))
    assert got[0] is None and got[2] is None and tuple(got[1].shape) == tuple(t["values"].shape)
    # an output the loss does not use arrives as None: T alone reaches the opacities alone
    op, va = t["faces_opacity"].clone().requires_grad_(True), t["values"].clone().requires_grad_(True)
    image, T = FG.composite_values_fused(Fragments(t["face"], None, None), op, va)
    g_op, g_va = th.autograd.grad(T.sum(), [op, va], allow_unused=True)
    assert g_op is not None and (g_va is None or float(g_va.abs().max()) == 0.0)
    # a non-contiguous values tensor is made contiguous
    perm = t["values"].permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3)
    assert not perm.is_contiguous()
    i2, T2 = FG.composite_values_fused(Fragments(t["face"], None, None), t["faces_opacity"], perm)
    i1, T1 = FG.composite_values_fused(Fragments(t["face"], None, None), t["faces_opacity"], t["values"])
    assert th.equal(i1, i2) and th.equal(T1, T2)


@pytest.mark.parametrize("poison", (float("nan"), float("inf")), ids=("nan", "inf"))
def test_empty_slot_values_are_not_read(hip_device, poison):
    """(5) a NaN / an Inf in every empty slot of values -- ids of -1, ids past F, INT32_MAX and negative ids other than -1: image,
    T and all gradients are finite and equal the run without them bit for bit (the opacity and scale gradients too: each is
    summed in one workgroup's table: DC.POISON_FRAME), and dL_dvalues is an exact 0 there."""
    dev = hip_device
    K, C, size = DC.POISON
    d = dict(_lists(K, C, size, DC.POISON_FRAME))
    g = th.Generator().manual_seed(13)
    r = th.rand(d["face"].shape, generator=g)
    face = th.where(r < 0.05, th.full_like(d["face"], INT32_MAX), d["face"])
    face = th.where((r >= 0.05) & (r < 0.1), th.full_like(face, -7), face)
    face = th.where((r >= 0.1) & (r < 0.13), th.full_like(face, -INT32_MAX - 1), face)
    d["face"] = face
    empty = _empty(d)
    assert all(int((face == x).sum()) > 0 for x in (-1, INT32_MAX, -7, -INT32_MAX - 1)) and int((face >= 7).sum()) > 0
    clean = _values_fused(d, dev, True)
    d2 = dict(d, values=th.where(empty[:, :, None].expand_as(d["values"]), th.full_like(d["values"], poison), d["values"]))
    assert not bool(th.isfinite(d2["values"]).all())
    bad = _values_fused(d2, dev, True)
    for name, a, b in [("image", clean[0], bad[0]), ("T", clean[1], bad[1])] + [("dL_d" + k, clean[2][k], bad[2][k]) for k in GRADS_V]:
        print(f"\nvalues {poison} in empty slots: {name} finite {bool(th.isfinite(b).all())}, bit-equal to the run without {th.equal(a, b)}")
        assert bool(th.isfinite(b).all()) and th.equal(a, b), name
    assert float(bad[2]["values"].cpu()[empty[:, :, None].expand_as(d["values"])].abs().max()) == 0.0
    face_m = th.where(empty, th.full_like(face, -1), face)
    ref = _values_model(dict(d2, face=face_m), True)
    _check_values(f"values {poison} in empty slots", dict(d2, face=face_m), ref, bad)


def test_face_with_a_vertex_out_of_range(hip_device):
    """(5b) a face whose row of `faces` holds a vertex index outside [0, P) -- P, -1, INT32_MAX -- interpolates to an exact 0,
    gets an exact 0 in dL_dbary and scatters nothing into dL_dvert_attrs: the float64 model receives such a face's slots as -1
    (and rows it can index)."""
    K, C, size = DC.BAD_ROWS
    d = dict(_lists(K, C, size))
    F, P = SIZES[size]
    faces = d["faces"].clone()
    faces[2, 1], faces[3, 0], faces[5, 2] = P, -1, INT32_MAX
    bad = ((faces < 0) | (faces >= P)).any(1)
    held = (d["face"] >= 0) & (d["face"] < F)
    hit = held & bad[d["face"].clamp(0, F - 1).long()]
    assert int(bad.sum()) == 3 and int(hit.sum()) > 100 and int((held & ~hit).sum()) > 100
    d["faces"] = faces
    dm = dict(d, face=th.where(hit, th.full_like(d["face"], -1), d["face"]), faces=faces.clamp(0, P - 1))
    _check_interp(f"K {K} C {C} {size}, three faces with a vertex out of range", dm, _interp_model(dm), _interp_fused(d, hip_device))


def test_non_finite_upstreams_leave_empty_slots_zero(hip_device):
    """(5c) a NaN / an Inf in the upstreams: dL_dvalues and dL_dbary are still an exact 0 in empty slots (a literal 0, not 0 times the
    upstream)."""
    K, C, size = DC.BAD_ROWS
    d = dict(_lists(K, C, size))
    g = th.Generator().manual_seed(17)
    for k in ("g_image", "g_out"):
        r = th.rand(d[k].shape, generator=g)
        d[k] = th.where(r < 0.1, th.full_like(d[k], float("nan")), th.where(r < 0.2, th.full_like(d[k], float("inf")), d[k]))
    empty = _empty(d)
    assert bool(empty.any())
    _, _, gv = _values_fused(d, hip_device, True, want=("values",))
    _, gi = _interp_fused(d, hip_device, want=("bary",))
    assert not bool(th.isfinite(gv["values"]).all()) and not bool(th.isfinite(gi["bary"]).all())  # (the upstreams did arrive)
    assert float(gv["values"].cpu()[empty[:, :, None].expand_as(d["values"])].abs().max()) == 0.0
    assert float(gi["bary"].cpu()[empty[:, :, None].expand(-1, -1, 2, -1, -1)].abs().max()) == 0.0


@pytest.mark.parametrize("frame", EDGE_FRAMES, ids=["x".join(map(str, f)) for f in EDGE_FRAMES])
def test_frames(hip_device, frame):
    """(6) a view of whole tiles only, and views of one pixel: one live lane per workgroup, the other 255 through every merge
    and barrier with key -1."""
    K, C, size = DC.EDGE_K, DC.EDGE_C, "shared_keys"
    d = _lists(K, C, size, frame)
    _check_interp(f"frame {frame}", d, _interp_reference(K, C, size, frame), _interp_fused(d, hip_device))
    _check_values(f"frame {frame}", d, _values_reference(K, C, size, True, frame), _values_fused(d, hip_device, True))


@functools.lru_cache(maxsize=None)
def _merge_lists(C):
    """The merge-level lists of test_composite_fused_gpu._merge_lists: K = 6 on a 32 x 32 view, F = 5; slot j < 5 holds stripes of
    period 2 << j along either axis, so each butterfly level of shade_merge meets equal keys alone; slot 5 holds face 3 over
    every pixel.  Opacities in (0.05, 0.4), no empty slot, one-signed values and upstreams."""
    B, H, W = MERGE_FRAME
    g = th.Generator().manual_seed(79 + C)
    py, px = th.meshgrid(th.arange(H), th.arange(W), indexing="ij")
    face = th.empty(B, MERGE_K, H, W, dtype=th.int32)
    for j in range(5):
        face[:, j] = th.where(py < 16, (px >> j) & 1, (py >> j) & 1).to(th.int32)
    face[:, 5] = 3
    pos = lambda *s: th.rand(*s, generator=g) + 0.5
    return dict(face=face, bary=th.rand(B, MERGE_K, 2, H, W, generator=g) * 0.4 + 0.05, faces=th.randint(0, MERGE_P, (MERGE_F, 3), generator=g, dtype=th.int32),
                faces_opacity=0.05 + 0.35 * th.rand(MERGE_F, generator=g), vert_attrs=th.randn(MERGE_P, C, generator=g),
                face_scale=pos(B, MERGE_F), values=pos(B, MERGE_K, C, H, W), g_out=pos(B, MERGE_K, C, H, W), g_image=pos(B, C, H, W),
                g_T=pos(B, 1, H, W))


def test_merge_levels(hip_device):
    """(6) shade_merge's four levels one at a time, and one face over a whole tile, in both backward kernels; one-signed values
    and upstreams, so the sums cannot agree by cancellation (max |ref| of the vert_attrs, opacity and scale gradients > 1)."""
    d = _merge_lists(DC.MERGE_C)
    ri, rv = _interp_model(d), _values_model(d, True)
    assert float(np.abs(ri[1]["vert_attrs"]).max()) > 1 and float(np.abs(rv[2]["faces_opacity"]).max()) > 1 and float(np.abs(rv[2]["face_scale"]).max()) > 1
    _check_interp("merge levels", d, ri, _interp_fused(d, hip_device))
    _check_values("merge levels", d, rv, _values_fused(d, hip_device, True))


def _rendered(dev, r, t, args, name, K):
    """(7) on a renderer's lists (return_fragments=K, fragment_grads=True): composite_values_fused(interpolate_fused(verts_color))
    + T bg is the renderer's colour where count <= K (FWD_TOL absolute, the bound of the existing fragments tests; pixels whose
    list holds a face of opacity 1 left out, the tet renderer's one exception), and a loss on the hit points
    interpolate_fused(frag, faces, verts) gives the verts.grad of the same loss through fragments.interpolate."""
    verts = t["verts"].clone().requires_grad_(True)
    out = r(*(verts if k == "verts" else t[k] for k in args))
    color, frag = out[0], out[-1]
    assert frag.bary.requires_grad and tuple(frag.pix_to_face.shape)[1] == K
    col = FG.interpolate_fused(frag, t["faces"], t["verts_color"])
    comp, T = FG.composite_values_fused(frag, t["faces_opacity"], col, t["faces_intense"])
    mine = comp + T * t["bg"].view(1, 3, 1, 1)
    opaque = ((t["faces_opacity"][frag.pix_to_face.clamp(min=0).long()] == 1) & (frag.pix_to_face >= 0)).any(1)
    keep = ((frag.count <= K) & ~opaque)[:, None]
    assert bool(keep.any())
    e = float(((mine - color).detach().abs() * keep).max())
    print(f"\n{name}: composite_values_fused(interpolate_fused) + T bg vs the renderer's colour {e:.2e} ({int(keep.sum())} of {keep.numel()} pixels)")
    assert e <= FWD_TOL
    gp = th.randn(tuple(frag.pix_to_face.shape[:2]) + (3,) + tuple(frag.pix_to_face.shape[2:]), generator=th.Generator().manual_seed(11)).to(dev)
    pos_f = FG.interpolate_fused(frag, t["faces"], verts)
    pos_t = FG.interpolate(frag, t["faces"], verts)
    g_f, = th.autograd.grad((pos_f * gp).sum(), verts, retain_graph=True)
    g_t, = th.autograd.grad((pos_t * gp).sum(), verts)
    ep = rel_err(pos_f.detach().cpu().numpy(), pos_t.detach().cpu().numpy())
    eg = rel_err(g_f.cpu().numpy(), g_t.cpu().numpy())
    print(f"{name}: hit points {ep:.2e}; verts.grad fused vs interpolate {eg:.2e} (max |ref| {float(g_t.abs().max()):.3g})")
    assert float(g_t.abs().max()) > 0 and ep <= FWD_TOL and eg <= GRAD_TOL


def test_rendered_tri_lists(hip_device):
    import dmesh_renderer_amd as dmr
    dev, K, Hs, Ws = hip_device, 4, 80, 112
    t = {k: v.to(dev) for k, v in scenes.layered_sheets(4, 8, 1, Hs, Ws, seed=3, opacity=(0.1, 0.4)).items()}
    r = dmr.TriRenderer(dmr.TriRenderSettings(Hs, Ws, t["bg"]), return_fragments=K, fragment_grads=True)
    _rendered(dev, r, t, TRI_ARGS, "tri", K)


def test_rendered_tet_lists(hip_device):
    import dmesh_renderer_amd as dmr
    dev, K, Hs, Ws = hip_device, 4, 48, 72
    t = {k: v.to(dev) for k, v in scenes.kuhn_tets(2, 1, Hs, Ws, seed=5).items()}
    r = dmr.TetRenderer(dmr.TetRenderSettings(Hs, Ws, t["bg"], 0), return_fragments=K, fragment_grads=True)
    _rendered(dev, r, t, TET_ARGS, "tet", K)


def test_graph_capture(hip_device):
    """(8) forward + backward of the chain of (3) captured into one HIP graph and replayed twice, the second time over inputs
    rewritten in place: outputs and gradients equal the eager ones to sum_order_tol; the accumulated outputs are exactly 0
    where no tile wrote (vertices and faces no list holds)."""
    dev = hip_device
    K, C, size = DC.GRAPH
    d = dict(_lists(K, C, size))
    F, P = SIZES[size]
    spare_f, spare_p = F - 50, P - 50   # the last 50 faces are in no list, the last 50 vertices in no face
    d["face"] = th.where((d["face"] >= spare_f) & (d["face"] < F), d["face"] - 100, d["face"])
    d["faces"] = th.where(d["faces"] >= spare_p, d["faces"] - 100, d["faces"])
    t = {k: v.to(dev) for k, v in d.items()}
    lv = {k: t[k].clone().requires_grad_(True) for k in CHAIN_GRADS}

    def step():
        image, T = _chain(t, lv)
        return [image.detach(), T.detach()] + list(th.autograd.grad((image * t["g_image"]).sum() + (T * t["g_T"]).sum(), [lv[k] for k in CHAIN_GRADS]))

    names = ("image", "T") + CHAIN_GRADS

    def same(captured, eager, what):
        for k, a, b in zip(names, captured, eager):
            e = rel_err(a.cpu().numpy(), b.cpu().numpy())
            print(f"\ngraph replay vs eager, {what}, {k}: {e:.2e} (max |eager| {float(b.abs().max()):.3g})")
            assert float(b.abs().max()) > 0 and e <= sum_order_tol(k), (what, k, e)
        by = dict(zip(names, captured))
        assert float(by["faces_opacity"][spare_f:].abs().max()) == 0.0 and float(by["face_scale"][:, spare_f:].abs().max()) == 0.0
        assert float(by["vert_attrs"][spare_p:].abs().max()) == 0.0

    graph, captured, eager = capture_replay(step)
    for x in captured:
        x.fill_(1.0)
    replay(graph)
    same(captured, eager, "the captured inputs")
    g = th.Generator().manual_seed(5)
    with th.no_grad():
        lv["faces_opacity"].copy_((th.rand(F, generator=g) * 0.5 + 0.2).to(dev))
        lv["vert_attrs"].copy_(th.randn(P, C, generator=g).to(dev))
    replay(graph)
    fresh = [x.detach().clone() for x in step()]
    th.cuda.synchronize()
    same(captured, fresh, "inputs rewritten in place")
    assert rel_err(fresh[0].cpu().numpy(), eager[0].cpu().numpy()) > 1e-3  # (the new inputs are other inputs)


def all_cases():
    """(tag, {name: float64 reference}) of every case above that compares against a float64 model: what check_inputs must hold
    for (tests/test_deferred_cpu.py checks it without a GPU)."""
    def both(tag, K, C, size, frame, scales=(True,)):
        out_r, g_r = _interp_reference(K, C, size, frame)
        yield tag + " interpolate", dict(g_r, out=out_r)
        for s in scales:
            image_r, T_r, v_r = _values_reference(K, C, size, s, frame)
            yield tag + f" composite_values scale {s}", dict(v_r, image=image_r, T=T_r)
    for K in DC.LISTS_K:
        for C in DC.LISTS_C:
            for size in SIZES:
                yield from both(f"lists K{K} C{C} {size}", K, C, size, FRAME, (False, True))
    for K, C, size in DC.MATRIX:
        yield from both(f"matrix K{K} C{C} {size}", K, C, size, NEW_FRAME)
    for frame in EDGE_FRAMES:
        yield from both(f"frame {frame}", DC.EDGE_K, DC.EDGE_C, "shared_keys", frame)
    d = _merge_lists(DC.MERGE_C)
    out_r, g_r = _interp_model(d)
    yield "merge interpolate", dict(g_r, out=out_r)
    image_r, T_r, v_r = _values_model(d, True)
    yield "merge composite_values", dict(v_r, image=image_r, T=T_r)


def test_binding_refusals(hip_device):
    """The binding's own refusals, below fragments.py's: every case of shading_cases.binding_refusals("deferred") raises a
    RuntimeError with the message the binding gave before its argument builders were put together from shared checks
    (tests/golden/shading_refusals.json: a record of that binding on the GPU over the same cases).  One or two wrong arguments
    per call, at one pixel: no call reaches a kernel."""
    import json
    import os
    import shading_cases as SC
    from dmesh_renderer_amd import _C
    golden = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shading_refusals.json")))["binding"]["deferred"]
    cases = SC.binding_refusals("deferred", hip_device)
    assert sorted({case for case, _, _ in cases}) == sorted(golden)
    for case, call, args in cases:
        with pytest.raises(RuntimeError) as e:
            getattr(_C, call)(*args)
        assert str(e.value) == golden[case], (case, call)
