"""fragments.face_visibility_fused on the GPU (csrc/dmr_visibility.hip: k_face_visibility, k_face_visibility_backward) against
fragments.face_visibility / fragments.face_coverage evaluated in float64 on the CPU, on the same float32 inputs cast up, ids
past F set to -1 for the model.

Bounds (the project's own): vis rel_err <= FWD_TOL = 1e-5 (scenes.rel_err), max_weight 1e-5 absolute, pixels exact, gradients
rel_err <= GRAD_TOL = 1e-4; two evaluations of the same sums in another order <= sum_order_tol(name).  Over these frames a
face's sum is a tile partial formed in f64 and at most six float32 atomics: a few 1e-7 of the largest entry.  Every case
prints what it measured (pytest -s).
"""
import functools

import numpy as np
import pytest
import torch as th

from dmesh_renderer_amd import Fragments, scenes
from dmesh_renderer_amd import fragments as FG
from harness import TET_ARGS, TRI_ARGS, capture_replay, replay
from shading_cases import EDGE_FRAMES, FRAME, MERGE_F, MERGE_FRAME, MERGE_K, NEW_FRAME, SIZES, kmax_of, smallest_k
from util import rel_err, sum_order_tol

pytestmark = pytest.mark.gpu

FWD_TOL = 1e-5
GRAD_TOL = 1e-4
INT32_MAX = 2 ** 31 - 1
GRADS = ("faces_opacity", "pixel_weight")


@functools.lru_cache(maxsize=None)
def _lists(K, size, frame=FRAME):
    """Caller-made lists (CPU float32 / int32), as test_composite_fused_gpu._lists makes them: 15 % of the slots -1, 10 % ids
    past F, anywhere in a list; one face of opacity exactly 1 and one of opacity exactly 0, the others small enough that T_K
    is not 0 at K = 32; a signed pixel_weight and a signed upstream of vis."""
    B, H, W = frame
    F = SIZES[size][0]
    g = th.Generator().manual_seed(2000 * K + (F > 100) + 7 * H)
    face = th.randint(0, F, (B, K, H, W), generator=g, dtype=th.int32)
    r = th.rand(B, K, H, W, generator=g)
    face = th.where(r < 0.15, th.full_like(face, -1), face)
    face = th.where((r >= 0.15) & (r < 0.25), face + F + (face % 3) * 5, face)  # F, F + 5.., past the faces
    opacity = th.rand(F, generator=g) * (0.12 if K > 5 else 0.6) + 0.01
    opacity[1], opacity[4] = 1.0, 0.0
    weight = th.randn(B, H, W, generator=g)
    g_vis = th.randn(B, F, generator=g)
    return dict(face=face, faces_opacity=opacity, pixel_weight=weight, g_vis=g_vis)


def _model(d, with_weight):
    """float64 on the CPU -> vis, max_weight, pixels (numpy), {name: grad}.  Ids >= F are empty slots: -1 here."""
    F = d["faces_opacity"].shape[0]
    face = th.where(d["face"] >= F, th.full_like(d["face"], -1), d["face"])
    lv = {k: d[k].double().requires_grad_(True) for k in GRADS if with_weight or k != "pixel_weight"}
    frag = Fragments(face, None, None)
    vis = FG.face_visibility(frag, lv["faces_opacity"], F, lv.get("pixel_weight"))
    mx, px = FG.face_coverage(frag, lv["faces_opacity"], F)
    (vis * d["g_vis"].double()).sum().backward()
    return vis.detach().numpy(), mx.numpy(), px.numpy(), {k: v.grad.numpy() for k, v in lv.items()}


@functools.lru_cache(maxsize=None)
def _reference(K, size, with_weight, frame=FRAME):
    return _model(_lists(K, size, frame), with_weight)


def _fused(d, dev, with_weight, coverage=True, want=GRADS):
    """face_visibility_fused on the device, gradients of `want` only -> vis, max_weight, pixels (None without coverage), {name: grad}."""
    t = {k: v.to(dev) for k, v in d.items()}
    F = t["faces_opacity"].shape[0]
    names = [k for k in want if with_weight or k != "pixel_weight"]
    lv = {k: t[k].clone().requires_grad_(True) for k in names}
    out = FG.face_visibility_fused(Fragments(t["face"], None, None), lv.get("faces_opacity", t["faces_opacity"]), F,
                                   lv.get("pixel_weight", t["pixel_weight"]) if with_weight else None, coverage=coverage)
    vis, mx, px = out if coverage else (out, None, None)
    if coverage:
        assert vis.requires_grad == bool(names) and not mx.requires_grad and not px.requires_grad and px.dtype == th.int32
    grads = th.autograd.grad((vis * t["g_vis"]).sum(), [lv[k] for k in names]) if names else ()
    return vis.detach(), mx, px, dict(zip(names, grads))


def _check(tag, ref, got):
    """vis, max_weight, pixels and every gradient of `got` (device) against the float64 model `ref`."""
    vis_r, mx_r, px_r, g_r = ref
    vis, mx, px, g = got
    assert tuple(vis.shape) == vis_r.shape == tuple(mx.shape) == tuple(px.shape) and vis.dtype == mx.dtype == th.float32
    ev, em = rel_err(vis.cpu().numpy(), vis_r), float(np.abs(mx.cpu().numpy() - mx_r).max())
    print(f"\n{tag}: vis {ev:.2e} (max |vis| {np.abs(vis_r).max():.3g}) max_weight {em:.2e} pixels up to {int(px_r.max())}")
    assert float(np.abs(vis_r).max()) > 0 and int(px_r.max()) > 0
    assert ev <= FWD_TOL and em <= FWD_TOL
    assert np.array_equal(px.cpu().numpy().astype(np.int64), px_r.astype(np.int64))
    assert set(g) == set(g_r)
    for k, r in g_r.items():
        x = g[k].cpu().numpy()
        assert x.shape == r.shape and x.dtype == np.float32 and float(np.abs(r).max()) > 0
        e = rel_err(x, r)
        print(f"  dL_d{k} {e:.2e} (max |ref| {np.abs(r).max():.3g})")
        assert e <= GRAD_TOL, (k, e)


@pytest.mark.parametrize("with_weight", (False, True), ids=("no_weight", "weight"))
@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("K", (1, 5, 32))
def test_caller_made_lists(hip_device, K, size, with_weight):
    """(1) vis, max_weight, pixels and both gradients against the float64 model: F = 7 (every lane of a wave merges) and
    F = 6000 (a tile holds more faces than the table's 560 slots: rows leave with direct atomics), partial tiles in both axes.
    Measured on the MI355X over the 12 cases: vis <= 1.8e-7 (rel_err), max_weight <= 5.4e-8 absolute, pixels equal; rel_err of
    the gradients <= 2.3e-7 (faces_opacity), 1.9e-7 (pixel_weight)."""
    _check(f"K {K} {size} weight {with_weight}", _reference(K, size, with_weight), _fused(_lists(K, size), hip_device, with_weight))


@pytest.mark.parametrize("size", list(SIZES))
def test_without_coverage(hip_device, size):
    """(2) coverage=False (the kernel without the maximum and the count, where a slot of value 0 retires early) gives the vis of
    coverage=True, and the same gradients."""
    d = _lists(5, size)
    a, _, _, ga = _fused(d, hip_device, True, coverage=True)
    b, mx, px, gb = _fused(d, hip_device, True, coverage=False)
    assert mx is None and px is None and tuple(a.shape) == tuple(b.shape)
    e = rel_err(b.cpu().numpy(), a.cpu().numpy())
    print(f"\n{size}: vis without coverage vs with {e:.2e}")
    assert e <= sum_order_tol("vis")
    assert rel_err(b.cpu().numpy(), _reference(5, size, True)[0]) <= FWD_TOL
    for k in GRADS:
        assert rel_err(gb[k].cpu().numpy(), ga[k].cpu().numpy()) <= sum_order_tol(k), k


MATRIX_K = (4, 8, 9, 16, 17, 32)


@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("K", MATRIX_K)
def test_every_kmax(hip_device, K, size):
    """(3) every KMAX of the backward at K == KMAX (the last row of its T_k array) and at its smallest K (1 and 5: test (1)), on a
    17 x 33 view.  Measured on the MI355X over the 12 cases: vis <= 4.5e-7, max_weight <= 3.6e-8, gradients <= 1.5e-7."""
    assert {kmax_of(k) for k in MATRIX_K} == {4, 8, 16, 32} and {smallest_k(16), smallest_k(32)} <= set(MATRIX_K)
    _check(f"K {K} {size}", _reference(K, size, True, NEW_FRAME), _fused(_lists(K, size, NEW_FRAME), hip_device, True))


@functools.lru_cache(maxsize=None)
def _merge_lists():
    """The merge-level lists of test_composite_fused_gpu._merge_lists: K = 6 on a 32 x 32 view, F = 5; slot j < 5 holds stripes
    of period 2 << j along either axis, so each butterfly level of the merge meets equal keys alone; slot 5 holds face 3 over
    every pixel.  Opacities in (0.05, 0.4), no empty slot, one-signed weights and upstream."""
    B, H, W = MERGE_FRAME
    g = th.Generator().manual_seed(78)
    py, px = th.meshgrid(th.arange(H), th.arange(W), indexing="ij")
    face = th.empty(B, MERGE_K, H, W, dtype=th.int32)
    for j in range(5):
        face[:, j] = th.where(py < 16, (px >> j) & 1, (py >> j) & 1).to(th.int32)
    face[:, 5] = 3
    opacity = 0.05 + 0.35 * th.rand(MERGE_F, generator=g)
    return dict(face=face, faces_opacity=opacity, pixel_weight=th.rand(B, H, W, generator=g) + 0.5, g_vis=th.rand(B, MERGE_F, generator=g) + 0.5)


def test_merge_levels(hip_device):
    """(4) the merge's four levels one at a time (sum, maximum and count), and one face over whole tiles: its pixels are 256
    per tile and slot.  One-signed weights and upstream: the sums cannot agree by cancellation."""
    d = _merge_lists()
    ref = _model(d, True)
    got = _fused(d, hip_device, True)
    _check("merge levels", ref, got)
    B, H, W = MERGE_FRAME
    slots = int((d["face"][0, :, 0, 0] == 3).sum())
    assert slots == 1 and got[2][0, 3].item() == 256 * (H // 16) * (W // 16) * slots
    assert float(np.abs(ref[3]["faces_opacity"]).max()) > 1


@pytest.mark.parametrize("frame", EDGE_FRAMES, ids=["x".join(map(str, f)) for f in EDGE_FRAMES])
def test_frames(hip_device, frame):
    """(5) a view of whole tiles only, and views of one pixel: one live lane per workgroup, the other 255 through every merge
    and barrier with key -1."""
    _check(f"frame {frame}", _reference(5, "shared_keys", True, frame), _fused(_lists(5, "shared_keys", frame), hip_device, True))


def test_only_some_gradients_wanted(hip_device):
    """(6) each of the two gradients alone equals the two together; without an upstream of vis both are None; F == 0 gives
    empty tensors."""
    from dmesh_renderer_amd import _C
    dev = hip_device
    d = _lists(5, "shared_keys")
    _, _, _, g_all = _fused(d, dev, True)
    for k in GRADS:
        _, _, _, g = _fused(d, dev, True, want=(k,))
        e = rel_err(g[k].cpu().numpy(), g_all[k].cpu().numpy())
        print(f"\ndL_d{k} alone vs both: {e:.2e}")
        assert list(g) == [k] and e <= sum_order_tol(k), (k, e)
    t = {k: v.to(dev) for k, v in d.items()}
    op, pw = t["faces_opacity"].clone().requires_grad_(True), t["pixel_weight"].clone().requires_grad_(True)
    vis, mx, px = FG.face_visibility_fused(Fragments(t["face"], None, None), op, 7, pw, coverage=True)
    nothing = th.zeros((), device=dev, requires_grad=True)
    assert th.autograd.grad(nothing * 1 + mx.sum() + px.sum(), [op, pw], allow_unused=True) == (None, None)
    assert _C.face_visibility_backward(t["face"], t["faces_opacity"], t["pixel_weight"], t["g_vis"], (False, False)) == (None, None)
    # F == 0
    none = th.zeros(0, device=dev)
    vis, mx, px = FG.face_visibility_fused(Fragments(t["face"], None, None), none, 0, t["pixel_weight"], coverage=True)
    assert tuple(vis.shape) == tuple(mx.shape) == tuple(px.shape) == (2, 0) and vis.dtype == th.float32 and px.dtype == th.int32
    assert tuple(FG.face_visibility_fused(Fragments(t["face"], None, None), none, 0).shape) == (2, 0)


def _rendered(dev, frag, t, name):
    """(7) on a renderer's lists: the sum over the faces against H W - sum(T) per view (T from composite_fused on the same
    lists), the faces with pixels == 0 against the ids absent from the lists, faces_opacity.grad against the torch path.
    Measured on the MI355X: the sum 1.1e-5 of 2 211 (tri, bound 0.09), 5.7e-6 of 1 011 (tet); vis against the torch path 5.9e-7,
    faces_opacity.grad 5.0e-7."""
    B, K, H, W = frag.pix_to_face.shape
    F = t["faces_opacity"].shape[0]
    frag = Fragments(frag.pix_to_face, frag.bary.detach(), frag.count)
    op = t["faces_opacity"].clone().requires_grad_(True)
    vis, mx, px = FG.face_visibility_fused(frag, op, F, coverage=True)
    _, T = FG.composite_fused(frag, t["faces"], t["faces_opacity"], t["verts_color"])
    for b in range(B):
        e = abs(float(vis[b].detach().double().sum()) - (H * W - float(T[b].double().sum())))
        print(f"\n{name} view {b}: |sum vis - (H W - sum T)| {e:.2e} of {float(vis[b].detach().sum()):.1f}; {int((px[b] > 0).sum())} of {F} faces held")
        assert e <= 1e-5 * H * W
        held = th.unique(frag.pix_to_face[b])
        held = held[(held >= 0) & (held < F)].long()
        mask = th.zeros(F, dtype=th.bool, device=dev)
        mask[held] = True
        assert held.numel() > 0 and bool(((px[b] > 0) == mask).all())
        assert int(px[b].sum()) == int(((frag.pix_to_face[b] >= 0) & (frag.pix_to_face[b] < F)).sum())
    g_f, = th.autograd.grad(vis.sum(), op)
    op_t = t["faces_opacity"].clone().requires_grad_(True)
    vis_t = FG.face_visibility(frag, op_t, F)
    g_t, = th.autograd.grad(vis_t.sum(), op_t)
    mx_t, px_t = FG.face_coverage(frag, t["faces_opacity"], F)
    ev, eg = rel_err(vis.detach().cpu().numpy(), vis_t.detach().cpu().numpy()), rel_err(g_f.cpu().numpy(), g_t.cpu().numpy())
    print(f"{name}: vis fused vs torch {ev:.2e}; faces_opacity.grad {eg:.2e} (max |ref| {float(g_t.abs().max()):.3g})")
    assert ev <= FWD_TOL and eg <= GRAD_TOL and float((mx - mx_t).abs().max()) <= FWD_TOL and th.equal(px.long(), px_t)


def test_rendered_tri_lists(hip_device):
    import dmesh_renderer_amd as dmr
    dev = hip_device
    K, Hs, Ws = 8, 80, 112
    t = {k: v.to(dev) for k, v in scenes.layered_sheets(6, 8, 2, Hs, Ws, seed=3, opacity=(0.1, 0.4)).items()}
    out = dmr.TriRenderer(dmr.TriRenderSettings(Hs, Ws, t["bg"]), return_fragments=K)(*(t[k] for k in TRI_ARGS))
    _rendered(dev, out[-1], t, "tri")


def test_rendered_tet_lists(hip_device):
    import dmesh_renderer_amd as dmr
    dev = hip_device
    K, Hs, Ws = 12, 48, 72
    t = {k: v.to(dev) for k, v in scenes.kuhn_tets(3, 2, Hs, Ws, seed=5).items()}
    out = dmr.TetRenderer(dmr.TetRenderSettings(Hs, Ws, t["bg"], 0), return_fragments=K)(*(t[k] for k in TET_ARGS))
    assert int(out[-1].count.max()) > 0
    _rendered(dev, out[-1], t, "tet")


def test_graph_capture(hip_device):
    """(8) forward and backward captured into one HIP graph: the replay gives the eager results, and after the inputs are
    rewritten in place it reads the new pixel_weight and faces_opacity.  (Two replays: with hipMemsetAsync nodes zeroing the
    outputs the second left small non-zero words in max_weight and pixels where no tile writes; the unit zeroes with a kernel.)
    Measured on the MI355X: replay against eager vis 4.8e-8, faces_opacity 4.1e-8, the others equal."""
    dev = hip_device
    d = _lists(5, "table_overflow")
    t = {k: v.to(dev) for k, v in d.items()}
    F = t["faces_opacity"].shape[0]
    lv = {k: t[k].clone().requires_grad_(True) for k in GRADS}

    def step():
        vis, mx, px = FG.face_visibility_fused(Fragments(t["face"], None, None), lv["faces_opacity"], F, lv["pixel_weight"], coverage=True)
        return [vis.detach(), mx, px] + list(th.autograd.grad((vis * t["g_vis"]).sum(), [lv[k] for k in GRADS]))

    names = ("vis", "max_weight", "pixels") + GRADS

    def same(captured, eager, what):
        for k, a, b in zip(names, captured, eager):
            e = rel_err(a.double().cpu().numpy(), b.double().cpu().numpy())
            print(f"\ngraph replay vs eager, {what}, {k}: {e:.2e} (max |eager| {float(b.abs().max()):.3g})")
            assert float(b.abs().max()) > 0 and e <= sum_order_tol(k), (what, k, e)

    graph, captured, eager = capture_replay(step)
    for x in captured:
        x.zero_()
    replay(graph)
    same(captured, eager, "the captured inputs")
    g = th.Generator().manual_seed(5)
    with th.no_grad():
        lv["faces_opacity"].copy_((th.rand(F, generator=g) * 0.5 + 0.2).to(dev))
        lv["pixel_weight"].copy_(th.randn(d["pixel_weight"].shape, generator=g).to(dev))
    replay(graph)
    fresh = [x.detach().clone() for x in step()]
    th.cuda.synchronize()
    same(captured, fresh, "inputs rewritten in place")
    assert rel_err(fresh[0].cpu().numpy(), eager[0].cpu().numpy()) > 1e-3  # (the new inputs are other inputs)


@pytest.mark.parametrize("poison", (float("nan"), float("inf")), ids=("nan", "inf"))
def test_non_finite_opacity_and_huge_ids_stay_in_bounds(hip_device, poison):
    """(9) a face of non-finite opacity and ids of INT32_MAX: the calls return and the rows of the other faces are the model's.
    The poisoned face sits in its lists' last slot only (behind it everything would be poisoned in the model too); nothing is
    asserted about its own row, nor about the gradients, which it reaches through every slot before it."""
    dev, K, bad = hip_device, 5, 2
    d = dict(_lists(K, "shared_keys"))
    F = d["faces_opacity"].shape[0]
    g = th.Generator().manual_seed(9)
    face = th.where(d["face"] == bad, th.full_like(d["face"], -1), d["face"])
    face[:, K - 1] = th.where(th.rand(face[:, K - 1].shape, generator=g) < 0.3, th.full_like(face[:, K - 1], bad), face[:, K - 1])
    face = th.where(th.rand(face.shape, generator=g) < 0.05, th.full_like(face, INT32_MAX), face)
    face[:, K - 1] = th.where(face[:, K - 2] == INT32_MAX, th.full_like(face[:, K - 1], bad), face[:, K - 1])  # and right behind one
    opacity = d["faces_opacity"].clone()
    opacity[bad] = poison
    d.update(face=face, faces_opacity=opacity)
    assert int((face == INT32_MAX).sum()) > 0 and int((face[:, K - 1] == bad).sum()) > 0 and int((face[:, :K - 1] == bad).sum()) == 0
    vis_r, mx_r, px_r, _ = _model(d, True)
    t = {k: v.to(dev) for k, v in d.items()}
    lv = {k: t[k].clone().requires_grad_(True) for k in GRADS}
    vis, mx, px = FG.face_visibility_fused(Fragments(t["face"], None, None), lv["faces_opacity"], F, lv["pixel_weight"], coverage=True)
    grads = th.autograd.grad((vis * t["g_vis"]).sum(), [lv[k] for k in GRADS])
    th.cuda.synchronize()
    assert tuple(grads[0].shape) == (F,) and tuple(grads[1].shape) == tuple(d["pixel_weight"].shape)
    others = [f for f in range(F) if f != bad]
    assert np.isfinite(vis_r[:, others]).all()
    ev = rel_err(vis.detach().cpu().numpy()[:, others], vis_r[:, others])
    em = float(np.abs(mx.cpu().numpy()[:, others] - mx_r[:, others]).max())
    print(f"\nopacity {poison}: the other faces' vis {ev:.2e} max_weight {em:.2e}")
    assert ev <= FWD_TOL and em <= FWD_TOL and np.array_equal(px.cpu().numpy()[:, others], px_r[:, others])


def test_binding_refusals(hip_device):
    """The binding's own refusals, below fragments.py's: every case of shading_cases.binding_refusals("visibility") raises a
    RuntimeError with the message the binding gave before its argument builders were put together from shared checks
    (tests/golden/shading_refusals.json: a record of that binding on the GPU over the same cases).  One or two wrong arguments
    per call, at one pixel: no call reaches a kernel."""
    import json
    import os
    import shading_cases as SC
    from dmesh_renderer_amd import _C
    golden = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shading_refusals.json")))["binding"]["visibility"]
    cases = SC.binding_refusals("visibility", hip_device)
    assert sorted({case for case, _, _ in cases}) == sorted(golden)
    for case, call, args in cases:
        with pytest.raises(RuntimeError) as e:
            getattr(_C, call)(*args)
        assert str(e.value) == golden[case], (case, call)
