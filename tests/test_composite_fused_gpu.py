"""fragments.composite_fused on the GPU (csrc/dmr_shade.hip: k_composite_fragments, k_composite_fragments_backward) against
fragments.composite evaluated in float64 on the CPU, on the same float32 inputs cast up.

Bounds (the project's own): forward FWD_TOL = 1e-5 absolute, gradients rel_err <= GRAD_TOL = 1e-4 (scenes.rel_err); two
evaluations of the same sums in another order <= sum_order_tol(name).  Every case prints what it measured (pytest -s).
"""
import functools

import numpy as np
import pytest
import torch as th

import fragments_ref as FR
from dmesh_renderer_amd import Fragments, scenes
from dmesh_renderer_amd import fragments as FG
from harness import TET_ARGS, TRI_ARGS, capture_replay, replay
from shading_cases import (EDGE_FRAME_C, EDGE_FRAME_K, EDGE_FRAMES, FRAME, MERGE_F, MERGE_FRAME, MERGE_K, MERGE_P, NEW_FRAME, SHADE_C,
                           SHADE_GRAPH, SHADE_K, SHADE_MATRIX, SHADE_MERGE_C, SHADE_MISALIGNED, SHADE_ONLY_SOME, SIZES, one_float_in)
from util import rel_err, sum_order_tol

pytestmark = pytest.mark.gpu

FWD_TOL = FR.FWD_TOL
GRAD_TOL = 1e-4
B, H, W = FRAME  # partial tiles in both axes
GRADS = ("faces_opacity", "vert_attrs", "face_scale", "bary")
# SIZES (shading_cases): many lanes of a wave share a key (the merge path) / a tile holds more distinct vertex rows than the
# table's 560 slots


@functools.lru_cache(maxsize=None)
def _lists(K, C, size, frame=FRAME):
    """Caller-made lists (CPU float32 / int32): random face ids with -1 and ids >= F anywhere in a list, one face of opacity
    exactly 1 and one of opacity exactly 0, and the upstream gradients of the image and of T."""
    B, H, W = frame
    F, P = SIZES[size]
    g = th.Generator().manual_seed(1000 * K + 10 * C + (F > 100))
    face = th.randint(0, F, (B, K, H, W), generator=g, dtype=th.int32)
    r = th.rand(B, K, H, W, generator=g)
    face = th.where(r < 0.15, th.full_like(face, -1), face)
    face = th.where((r >= 0.15) & (r < 0.25), face + F + (face % 3) * 5, face)  # F, F + 5.., past the faces
    bary = th.rand(B, K, 2, H, W, generator=g) * 0.6 - 0.05
    faces = th.randint(0, P, (F, 3), generator=g, dtype=th.int32)
    # (opacities that leave something behind 32 slots: T_K ~ 0.93^24)
    opacity = th.rand(F, generator=g) * (0.12 if K > 5 else 0.6) + 0.01
    opacity[1], opacity[4] = 1.0, 0.0
    attrs = th.randn(P, C, generator=g)
    scale = th.rand(B, F, generator=g) + 0.5
    g_image = th.randn(B, C, H, W, generator=g)
    g_T = th.randn(B, 1, H, W, generator=g)
    return dict(face=face, bary=bary, faces=faces, faces_opacity=opacity, vert_attrs=attrs, face_scale=scale, g_image=g_image, g_T=g_T)


@functools.lru_cache(maxsize=None)
def _reference(K, C, size, with_scale, frame=FRAME):
    """fragments.composite in float64 on the CPU -> image, T, the four gradients (numpy).  Ids >= F are empty slots: -1 here."""
    return _model(_lists(K, C, size, frame), with_scale)


def _model(d, with_scale):
    F = d["faces"].shape[0]
    face = th.where(d["face"] >= F, th.full_like(d["face"], -1), d["face"])
    lv = {k: d[k].double().requires_grad_(True) for k in GRADS if with_scale or k != "face_scale"}
    image, T = FG.composite(Fragments(face, lv["bary"], None), d["faces"], lv["faces_opacity"], lv["vert_attrs"],
                            face_scale=lv.get("face_scale"))
    ((image * d["g_image"].double()).sum() + (T * d["g_T"].double()).sum()).backward()
    return image.detach().numpy(), T.detach().numpy(), {k: v.grad.numpy() for k, v in lv.items()}


def _fused(d, dev, with_scale, want=GRADS, g_image=True, g_T=True, leaves=None):
    """composite_fused on the device, gradients of `want` only -> image, T, {name: grad}.  leaves: {name: the device tensor to
    differentiate, as it is (its storage and offset)} in place of a fresh copy of d[name]."""
    t = {k: v.to(dev) for k, v in d.items()}
    names = [k for k in want if with_scale or k != "face_scale"]
    lv = {k: (leaves[k].detach() if leaves and k in leaves else t[k].clone()).requires_grad_(True) for k in names}
    image, T = FG.composite_fused(Fragments(t["face"], lv.get("bary", t["bary"]), None), t["faces"], lv.get("faces_opacity", t["faces_opacity"]),
                                  lv.get("vert_attrs", t["vert_attrs"]), face_scale=lv.get("face_scale", t["face_scale"]) if with_scale else None)
    loss = 0
    if g_image is not False:
        loss = loss + (image * (t["g_image"] if g_image is True else g_image)).sum()
    if g_T is not False:
        loss = loss + (T * (t["g_T"] if g_T is True else g_T)).sum()
    grads = th.autograd.grad(loss, [lv[k] for k in names])
    return image.detach(), T.detach(), dict(zip(names, grads))


@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("with_scale", (False, True), ids=("no_scale", "scale"))
@pytest.mark.parametrize("C", SHADE_C)
@pytest.mark.parametrize("K", SHADE_K)
def test_caller_made_lists(hip_device, K, C, with_scale, size):
    """(a) image, T and all four gradients against the float64 model.
    Measured on the MI355X over the 48 cases: image <= 5.0e-7, T <= 1.9e-7 absolute; rel_err of the gradients <= 4.3e-7
    (faces_opacity), 2.3e-7 (vert_attrs), 2.2e-7 (face_scale), 1.8e-7 (bary)."""
    d = _lists(K, C, size)
    image_r, T_r, g_r = _reference(K, C, size, with_scale)
    image, T, g = _fused(d, hip_device, with_scale)
    assert tuple(image.shape) == (B, C, H, W) and tuple(T.shape) == (B, 1, H, W)
    ei, eT = float(np.abs(image.cpu().numpy() - image_r).max()), float(np.abs(T.cpu().numpy() - T_r).max())
    print(f"\nK {K} C {C} {size} scale {with_scale}: image {ei:.2e} T {eT:.2e} (max |image| {np.abs(image_r).max():.3g})")
    assert ei <= FWD_TOL and eT <= FWD_TOL
    assert set(g) == set(g_r)
    for k, ref in g_r.items():
        got = g[k].cpu().numpy()
        assert got.shape == ref.shape and got.dtype == np.float32
        e = rel_err(got, ref)
        print(f"  dL_d{k} {e:.2e} (max |ref| {np.abs(ref).max():.3g})")
        assert e <= GRAD_TOL, (k, e)
    # empty slots: exact zeros in dL/dbary
    F = d["faces"].shape[0]
    empty = ((d["face"] < 0) | (d["face"] >= F))[:, :, None].expand(-1, -1, 2, -1, -1)
    assert float(g["bary"].cpu()[empty].abs().max()) == 0.0


def test_only_some_gradients_wanted(hip_device):
    """(b) each of the four alone equals the four together; a backward with only T's upstream equals one with a zero image
    upstream beside it, one with only the image's equals one with a zero upstream of T, and the two add up to the model's
    gradients.  Two evaluations of the same sums: sum_order_tol."""
    K, C, size = SHADE_ONLY_SOME
    d = _lists(K, C, size)
    dev = hip_device
    _, _, g_all = _fused(d, dev, True)
    for k in GRADS:
        _, _, g = _fused(d, dev, True, want=(k,))
        e = rel_err(g[k].cpu().numpy(), g_all[k].cpu().numpy())
        print(f"\ndL_d{k} alone vs all four: {e:.2e}")
        assert list(g) == [k] and e <= sum_order_tol(k), (k, e)
    _, _, g_T = _fused(d, dev, True, g_image=False)
    _, _, g_T0 = _fused(d, dev, True, g_image=th.zeros_like(d["g_image"]).to(dev))
    _, _, g_I = _fused(d, dev, True, g_T=False)
    _, _, g_I0 = _fused(d, dev, True, g_T=th.zeros_like(d["g_T"]).to(dev))
    _, _, ref = _reference(K, C, size, True)
    for k in GRADS:
        e = rel_err(g_T[k].cpu().numpy(), g_T0[k].cpu().numpy())
        e2 = rel_err((g_T[k] + g_I[k]).cpu().numpy(), ref[k])
        e1 = rel_err(g_I[k].cpu().numpy(), g_I0[k].cpu().numpy())
        print(f"dL_d{k}: only grad_T vs zero grad_image {e:.2e}; only grad_image vs zero grad_T {e1:.2e}; the two summed vs the model {e2:.2e}")
        assert e <= sum_order_tol(k) and e1 <= sum_order_tol(k) and e2 <= GRAD_TOL, (k, e, e1, e2)
    for k in ("vert_attrs", "face_scale", "bary"):  # T depends on the opacities alone
        assert float(g_T[k].abs().max()) == 0.0, k


def test_rendered_tri_lists(hip_device):
    """(c) composite_fused + T bg is the tri renderer's colour where count <= K; a loss on the hit positions
    composite_fused(frag, faces, opacity, verts) gives the verts.grad of the same loss through composite (fragment_grads: the
    gradient of bary goes on into the renderer's backward).
    Measured on the MI355X: colour 8.9e-8, hit positions 1.2e-7, verts.grad 4.1e-7 (max |ref| 3.62)."""
    import dmesh_renderer_amd as dmr
    dev = hip_device
    K, Hs, Ws = 8, 80, 112
    d = scenes.layered_sheets(6, 8, 1, Hs, Ws, seed=3, opacity=(0.1, 0.4))
    t = {k: v.to(dev) for k, v in d.items()}
    r = dmr.TriRenderer(dmr.TriRenderSettings(Hs, Ws, t["bg"]), return_fragments=K, fragment_grads=True)
    verts = t["verts"].clone().requires_grad_(True)
    color, depth, frag = r(*(verts if k == "verts" else t[k] for k in TRI_ARGS))
    assert frag.bary.requires_grad
    comp, T = FG.composite_fused(frag, t["faces"], t["faces_opacity"], t["verts_color"], face_scale=t["faces_intense"])
    mine = comp + T * t["bg"].view(1, 3, 1, 1)
    keep = (frag.count <= K)[:, None]
    assert bool(keep.any())
    e = float(((mine - color).detach().abs() * keep).max())
    print(f"\ncomposite_fused + T bg vs the renderer's colour {e:.2e} ({int(keep.sum())} of {keep.numel()} pixels)")
    assert e <= FWD_TOL
    gp = th.randn(1, 3, Hs, Ws, generator=th.Generator().manual_seed(11)).to(dev)
    pos_f, _ = FG.composite_fused(frag, t["faces"], t["faces_opacity"], verts)
    pos_c, _ = FG.composite(frag, t["faces"], t["faces_opacity"], verts)
    g_f, = th.autograd.grad((pos_f * gp).sum(), verts, retain_graph=True)
    g_c, = th.autograd.grad((pos_c * gp).sum(), verts)
    ep = float((pos_f - pos_c).detach().abs().max())
    eg = rel_err(g_f.cpu().numpy(), g_c.cpu().numpy())
    print(f"hit positions {ep:.2e}; verts.grad fused vs composite {eg:.2e} (max |ref| {float(g_c.abs().max()):.3g})")
    assert ep <= FWD_TOL and eg <= GRAD_TOL


def test_rendered_tet_lists(hip_device):
    """(d) forward on the tet renderer's lists (march order, unclamped barycentrics).  Measured on the MI355X: image 1.2e-7, T 0 (deepest
    list 17 of K = 12 slots: the truncated sums agree)."""
    import dmesh_renderer_amd as dmr
    dev = hip_device
    K, Hs, Ws = 12, 48, 72
    d = scenes.kuhn_tets(3, 2, Hs, Ws, seed=5)
    t = {k: v.to(dev) for k, v in d.items()}
    out = dmr.TetRenderer(dmr.TetRenderSettings(Hs, Ws, t["bg"], 0), return_fragments=K)(*(t[k] for k in TET_ARGS))
    frag = out[-1]
    assert int(frag.count.max()) > 0
    a, Ta = FG.composite_fused(frag, t["faces"], t["faces_opacity"], t["verts_color"], face_scale=t["faces_intense"])
    b, Tb = FG.composite(frag, t["faces"], t["faces_opacity"], t["verts_color"], face_scale=t["faces_intense"])
    e, eT = float((a - b).abs().max()), float((Ta - Tb).abs().max())
    print(f"\ntet lists, fused vs composite: image {e:.2e} T {eT:.2e} (deepest list {int(frag.count.max())})")
    assert e <= FWD_TOL and eT <= FWD_TOL


def test_graph_capture(hip_device):
    """(e) one forward + backward captured into a HIP graph and replayed: the replayed gradients are the eager ones."""
    K, C, size = SHADE_GRAPH
    d = _lists(K, C, size)
    dev = hip_device
    t = {k: v.to(dev) for k, v in d.items()}
    lv = [t[k].clone().requires_grad_(True) for k in GRADS]

    def step():
        image, T = FG.composite_fused(Fragments(t["face"], lv[3], None), t["faces"], lv[0], lv[1], face_scale=lv[2])
        return list(th.autograd.grad((image * t["g_image"]).sum() + (T * t["g_T"]).sum(), lv))

    graph, captured, eager = capture_replay(step)
    for x in captured:
        x.zero_()
    replay(graph)
    for k, a, b in zip(GRADS, captured, eager):
        e = rel_err(a.cpu().numpy(), b.cpu().numpy())
        print(f"\ngraph replay vs eager dL_d{k}: {e:.2e} (max |eager| {float(b.abs().max()):.3g})")
        assert float(b.abs().max()) > 0 and e <= sum_order_tol(k), (k, e)


# ---------------------------------------------------------------------------
# Every instantiation (shading_cases: the tables below and what each row reaches; tests/test_shading_coverage_cpu.py checks
# without a GPU that together they reach all 20, and that every case here meets check_inputs).
# ---------------------------------------------------------------------------
def check_inputs(d, ref, signed=True):
    """What a case's inputs must give before anything is compared: a non-zero reference for every gradient (an all-empty list
    cannot pass), and, under a one-signed upstream, opacity and scale gradients that no cancellation made small."""
    _, _, g_r = ref
    for k, r in g_r.items():
        assert float(np.abs(r).max()) > 0, k
    if not signed:
        assert float(np.abs(g_r["faces_opacity"]).max()) > 1 and float(np.abs(g_r["face_scale"]).max()) > 1


def _check(tag, d, ref, got, signed=True):
    """image, T and every gradient of `got` (device) against the float64 model `ref`, as test_caller_made_lists does."""
    check_inputs(d, ref, signed)
    image_r, T_r, g_r = ref
    image, T, g = got
    assert tuple(image.shape) == image_r.shape and tuple(T.shape) == T_r.shape
    ei, eT = float(np.abs(image.cpu().numpy() - image_r).max()), float(np.abs(T.cpu().numpy() - T_r).max())
    print(f"\n{tag}: image {ei:.2e} T {eT:.2e} (max |image| {np.abs(image_r).max():.3g})")
    assert ei <= FWD_TOL and eT <= FWD_TOL
    assert set(g) == set(g_r)
    for k, r in g_r.items():
        x = g[k].cpu().numpy()
        assert x.shape == r.shape and x.dtype == np.float32
        e = rel_err(x, r)
        print(f"  dL_d{k} {e:.2e} (max |ref| {np.abs(r).max():.3g})")
        assert e <= GRAD_TOL, (k, e)
    F = d["faces"].shape[0]
    empty = ((d["face"] < 0) | (d["face"] >= F))[:, :, None].expand(-1, -1, 2, -1, -1)
    if bool(empty.any()):  # empty slots: exact zeros in dL/dbary
        assert float(g["bary"].cpu()[empty].abs().max()) == 0.0


@functools.lru_cache(maxsize=None)
def _merge_lists(C):
    """K = 6 on a 32 x 32 view, F = 5.  Slot j < 5 holds face (px >> j) & 1 in the rows py < 16 and (py >> j) & 1 below: stripes of
    period 2, 4, 8, 16, 32 along either axis, so each butterfly level of shade_merge meets equal keys alone, whichever lanes
    FragSlots gives a pixel's neighbours.  Slot 5: one face over every pixel (the real workload's most common tile: the most
    retirements, 16 rows adding into one f64 cell).  Opacities in (0.05, 0.4), no empty slot, one-signed upstreams."""
    B, H, W = MERGE_FRAME
    g = th.Generator().manual_seed(77 + C)
    py, px = th.meshgrid(th.arange(H), th.arange(W), indexing="ij")
    face = th.empty(B, MERGE_K, H, W, dtype=th.int32)
    for j in range(5):
        face[:, j] = th.where(py < 16, (px >> j) & 1, (py >> j) & 1).to(th.int32)
    face[:, 5] = 3
    bary = th.rand(B, MERGE_K, 2, H, W, generator=g) * 0.6 - 0.05
    faces = th.randint(0, MERGE_P, (MERGE_F, 3), generator=g, dtype=th.int32)
    opacity = 0.05 + 0.35 * th.rand(MERGE_F, generator=g)
    assert bool(((opacity > 0.05) & (opacity < 0.4)).all())
    attrs = th.randn(MERGE_P, C, generator=g)
    scale = th.rand(B, MERGE_F, generator=g) + 0.5
    g_image = th.rand(B, C, H, W, generator=g) + 0.5
    g_T = th.rand(B, 1, H, W, generator=g) + 0.5
    return dict(face=face, bary=bary, faces=faces, faces_opacity=opacity, vert_attrs=attrs, face_scale=scale, g_image=g_image, g_T=g_T)


@functools.lru_cache(maxsize=None)
def _merge_reference(C):
    return _model(_merge_lists(C), True)


def new_cases():
    """(tag, lists, float64 reference, one-signed upstream) of every case below: what check_inputs must hold for."""
    for K, C, with_scale, size in SHADE_MATRIX:
        yield f"matrix K{K} C{C} {size} scale {with_scale}", _lists(K, C, size, NEW_FRAME), _reference(K, C, size, with_scale, NEW_FRAME), True
    for K, C in SHADE_MISALIGNED:
        yield f"misaligned K{K} C{C}", _lists(K, C, "table_overflow", NEW_FRAME), _reference(K, C, "table_overflow", True, NEW_FRAME), True
    yield "merge levels", _merge_lists(SHADE_MERGE_C), _merge_reference(SHADE_MERGE_C), False
    for frame in EDGE_FRAMES:
        yield (f"frame {frame}", _lists(EDGE_FRAME_K, EDGE_FRAME_C, "shared_keys", frame),
               _reference(EDGE_FRAME_K, EDGE_FRAME_C, "shared_keys", True, frame), True)


@pytest.mark.parametrize("K,C,with_scale,size", SHADE_MATRIX,
                         ids=[f"K{K}-C{C}-{'scale' if s else 'no_scale'}-{size}" for K, C, s, size in SHADE_MATRIX])
def test_instantiation_matrix(hip_device, K, C, with_scale, size):
    """(f) the backward's KMAX = 16 kernels, K == KMAX at 4, 8 and 16, the first K of the next instantiation (9, 17), and the
    float4 row loads (C % 4 == 0) with the forward's CH 16 guard at C = 20 and both walks at SHADE_MAX_C: image, T and all four
    gradients against the float64 model, on a 17 x 33 view.
    Measured on the MI355X over the 27 cases: image <= 4.8e-7, T <= 1.9e-7 absolute; rel_err of the gradients <= 3.2e-7
    (faces_opacity), 1.5e-7 (vert_attrs), 8.8e-7 (face_scale), 2.4e-7 (bary)."""
    d = _lists(K, C, size, NEW_FRAME)
    _check(f"K {K} C {C} {size} scale {with_scale}", d, _reference(K, C, size, with_scale, NEW_FRAME), _fused(d, hip_device, with_scale))


@pytest.mark.parametrize("K,C", SHADE_MISALIGNED, ids=[f"K{K}-C{C}" for K, C in SHADE_MISALIGNED])
def test_misaligned_base(hip_device, K, C):
    """(g) C % 4 == 0 with vert_attrs one float into a larger buffer: the binding's .contiguous() keeps that pointer, so the
    scalar loads run (vec = 0) where the same values in a buffer of their own take the float4 loads.  Both against the float64
    model, and against each other (forward FWD_TOL; gradients: the same sums in another order, sum_order_tol).
    Measured on the MI355X over the 3 cases, either call against the model: image, T <= 1.6e-7, gradients <= 1.7e-7; misaligned
    against aligned: the forward bit-equal, dL_dfaces_opacity 6.8e-8, dL_dvert_attrs 3.0e-8, dL_dface_scale 5.1e-8, dL_dbary 0."""
    dev, size = hip_device, "table_overflow"
    d = _lists(K, C, size, NEW_FRAME)
    ref = _reference(K, C, size, True, NEW_FRAME)
    off, own = one_float_in(d["vert_attrs"].to(dev)), d["vert_attrs"].to(dev).clone()
    assert off.is_contiguous() and off.data_ptr() % 16 == 4 and own.data_ptr() % 16 == 0
    assert bool((off == own).all())
    got = _fused(d, dev, True, leaves={"vert_attrs": off})
    _check(f"K {K} C {C} misaligned", d, ref, got)
    alg = _fused(d, dev, True, leaves={"vert_attrs": own})
    _check(f"K {K} C {C} aligned", d, ref, alg)
    ei, eT = float((got[0] - alg[0]).abs().max()), float((got[1] - alg[1]).abs().max())
    print(f"misaligned vs aligned: image {ei:.2e} T {eT:.2e}; forward bit-equal: {bool(th.equal(got[0], alg[0]) and th.equal(got[1], alg[1]))}")
    assert ei <= FWD_TOL and eT <= FWD_TOL
    for k in GRADS:
        e = rel_err(got[2][k].cpu().numpy(), alg[2][k].cpu().numpy())
        print(f"  dL_d{k} misaligned vs aligned {e:.2e}")
        assert e <= sum_order_tol(k), (k, e)


def test_merge_levels(hip_device):
    """(h) shade_merge's four levels one at a time, and one face over a whole tile (_merge_lists), against the float64 model;
    the upstreams are one-signed, so the opacity and scale gradients (max |ref| > 1, asserted) cannot agree by cancellation.
    Measured on the MI355X: image 3.9e-7, T 3.1e-8; dL_dfaces_opacity 1.5e-7, dL_dvert_attrs 4.3e-8, dL_dface_scale 7.5e-8,
    dL_dbary 1.5e-7."""
    d = _merge_lists(SHADE_MERGE_C)
    _check(f"merge levels K {MERGE_K} C {SHADE_MERGE_C}", d, _merge_reference(SHADE_MERGE_C), _fused(d, hip_device, True), signed=False)


@pytest.mark.parametrize("frame", EDGE_FRAMES, ids=["x".join(map(str, f)) for f in EDGE_FRAMES])
def test_frames(hip_device, frame):
    """(i) a view of whole tiles only, and views of one pixel: one live lane per workgroup, the other 255 through every merge
    and barrier with key -1.
    Measured on the MI355X over both: image <= 2.0e-7, T <= 6.0e-8; gradients <= 2.3e-7 (face_scale)."""
    K, C, size = EDGE_FRAME_K, EDGE_FRAME_C, "shared_keys"
    d = _lists(K, C, size, frame)
    _check(f"frame {frame} K {K} C {C}", d, _reference(K, C, size, True, frame), _fused(d, hip_device, True))


def test_binding_refusals(hip_device):
    """The binding's own refusals, below fragments.py's: every case of shading_cases.binding_refusals("shade") raises a
    RuntimeError with the message the binding had before its list checks were merged (tests/golden/shading_refusals.json:
    copied from that source text and compared with a run of that binding over the same cases).
    One wrong argument per call, at one pixel: no call reaches a kernel."""
    import json
    import os
    import shading_cases as SC
    from dmesh_renderer_amd import _C
    golden = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shading_refusals.json")))["binding"]["shade"]
    cases = SC.binding_refusals("shade", hip_device)
    assert sorted({case for case, _, _ in cases}) == sorted(golden)
    for case, call, args in cases:
        with pytest.raises(RuntimeError) as e:
            getattr(_C, call)(*args)
        assert str(e.value) == golden[case], (case, call)
