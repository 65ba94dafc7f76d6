"""fragments.composite_texture_fused on the GPU (csrc/dmr_texture.hip: k_composite_texture, k_composite_texture_backward)
against fragments.composite_texture evaluated in float64 on the CPU, on the same float32 inputs cast up.

Bounds: gradients rel_err <= GRAD_TOL = 1e-4 (scenes.rel_err), T <= FWD_TOL = 1e-5 absolute; the image max(FWD_TOL, 4 x the
deviation of the model evaluated in float32 on the CPU from the model in float64) -- the formula's own float32 noise (the
sample coordinate s Wt - 0.5 is rounded at a magnitude of up to 2 Wt, and the texel difference multiplies that), computed by
each test from the model alone, the rule tests/test_tet_fragments_gpu.py uses for its barycentrics; two evaluations of the
same sums in another order <= sum_order_tol(name).

The UV and barycentric gradients jump where a sample sits on a texel-centre line (the cell is a constant of the model), and
the float32 coordinate differs from the float64 one by up to ~3e-5 texel: every slot whose float64 x or y lies within 1e-3
of an integer is emptied before either side sees the lists (at most 2 % of the used slots, asserted).
Every case prints what it measured (pytest -s).
"""
import functools

import numpy as np
import pytest
import torch as th

import fragments_ref as FR
from dmesh_renderer_amd import Fragments, scenes
from dmesh_renderer_amd import fragments as FG
from harness import TRI_ARGS, capture_replay, replay
from shading_cases import (EDGE_FRAME_C, EDGE_FRAME_K, EDGE_FRAMES, FRAME, MERGE_F, MERGE_FRAME, MERGE_K, MERGE_P, NEW_FRAME, SIZES,
                           TEXTURE_CASES, TEXTURE_EDGE_FRAME, TEXTURE_GRAPH, TEXTURE_MATRIX, TEXTURE_MERGE, TEXTURE_MISALIGNED,
                           TEXTURE_NO_TEX_GRAD, TEXTURE_ONLY_SOME, one_float_in)
from util import rel_err, sum_order_tol

pytestmark = pytest.mark.gpu

FWD_TOL = FR.FWD_TOL
GRAD_TOL = 1e-4
LINE_BAND = 1e-3
B, H, W = FRAME  # partial tiles in both axes
GRADS = ("faces_opacity", "vert_uvs", "texture", "face_scale", "bary")
# SIZES (shading_cases), (F, Pu): many lanes of a wave share a key (the merge path, a handful of table cells) / a tile holds
# more distinct UV rows than the 560 cells of that table and, with the 32 x 48 texture, fills the texel table to its probe limit
# at K = 5 (about 1400 of the 1536 texels against 1408 cells) and past its size at K = 32 (1024 cells): rows leave with direct
# atomics


def _sample_xy(face, bary, corners, uvs, Ht, Wt):
    """float64 (x, y) of every slot (whatever its face id: ids outside [0, F) read face 0)."""
    F = corners.shape[0]
    idx = th.where((face >= 0) & (face < F), face, th.zeros_like(face)).long()
    uv = uvs.double()[corners.long()[idx]]
    u, v = bary[:, :, 0].double(), bary[:, :, 1].double()
    st = (th.stack([1 - u - v, u, v], -1).unsqueeze(-1) * uv).sum(-2)
    return st[..., 0] * Wt - 0.5, st[..., 1] * Ht - 0.5


def _off_the_lines(face, bary, corners, uvs, Ht, Wt):
    """face with -1 in every used slot whose sample lies within LINE_BAND of a texel-centre line, and the share removed."""
    F = corners.shape[0]
    x, y = _sample_xy(face, bary, corners, uvs, Ht, Wt)
    used = (face >= 0) & (face < F)
    near = used & (((x - x.round()).abs() < LINE_BAND) | ((y - y.round()).abs() < LINE_BAND))
    share = float(near.sum()) / max(1, int(used.sum()))
    return th.where(near, th.full_like(face, -1), face), share


@functools.lru_cache(maxsize=None)
def _lists(K, C, tex, size, with_uvf, frame=FRAME):
    """Caller-made lists (CPU float32 / int32), as test_composite_fused_gpu makes them: random face ids with -1 and ids >= F
    anywhere in a list, one face of opacity exactly 1 and one of opacity exactly 0; UVs in [-1, 2] (both wraps act on both
    sides); the upstream gradients of the image and of T.  Slots near a texel-centre line are already emptied."""
    B, H, W = frame
    F, Pu = SIZES[size]
    Ht, Wt = tex
    g = th.Generator().manual_seed(1000 * K + 10 * C + (F > 100) + 100000 * Wt)
    face = th.randint(0, F, (B, K, H, W), generator=g, dtype=th.int32)
    r = th.rand(B, K, H, W, generator=g)
    face = th.where(r < 0.15, th.full_like(face, -1), face)
    face = th.where((r >= 0.15) & (r < 0.25), face + F + (face % 3) * 5, face)  # F, F + 5.., past the faces
    bary = th.rand(B, K, 2, H, W, generator=g) * 0.6 - 0.05
    faces = th.randint(0, Pu, (F, 3), generator=g, dtype=th.int32)
    uv_faces = th.randint(0, Pu, (F, 3), generator=g, dtype=th.int32) if with_uvf else None
    opacity = th.rand(F, generator=g) * (0.12 if K > 5 else 0.6) + 0.01
    opacity[1], opacity[4] = 1.0, 0.0
    uvs = th.rand(Pu, 2, generator=g) * 3 - 1
    texture = th.randn(Ht, Wt, C, generator=g)
    scale = th.rand(B, F, generator=g) + 0.5
    g_image = th.randn(B, C, H, W, generator=g)
    g_T = th.randn(B, 1, H, W, generator=g)
    face, share = _off_the_lines(face, bary, faces if uv_faces is None else uv_faces, uvs, Ht, Wt)
    return dict(face=face, bary=bary, faces=faces, uv_faces=uv_faces, faces_opacity=opacity, vert_uvs=uvs, texture=texture,
                face_scale=scale, g_image=g_image, g_T=g_T, removed=share)


def _model(d, wrap, with_scale, dtype, grads=True):
    """fragments.composite_texture on the CPU in `dtype` -> image, T, the five gradients (numpy).  Ids >= F are empty: -1 here."""
    F = d["faces"].shape[0]
    face = th.where(d["face"] >= F, th.full_like(d["face"], -1), d["face"])
    lv = {k: d[k].to(dtype).requires_grad_(grads) for k in GRADS if with_scale or k != "face_scale"}
    image, T = FG.composite_texture(Fragments(face, lv["bary"], None), d["faces"], lv["faces_opacity"], lv["vert_uvs"], lv["texture"],
                                    lv.get("face_scale"), uv_faces=d["uv_faces"], wrap=wrap)
    if not grads:
        return image.numpy(), T.numpy(), {}
    ((image * d["g_image"].to(dtype)).sum() + (T * d["g_T"].to(dtype)).sum()).backward()
    return image.detach().numpy(), T.detach().numpy(), {k: v.grad.numpy() for k, v in lv.items()}


@functools.lru_cache(maxsize=None)
def _reference(K, C, tex, size, with_uvf, wrap, with_scale, frame=FRAME):
    """The float64 model and the image bound: max(FWD_TOL, 4 x |model in float32 - model in float64|)."""
    return _reference_of(_lists(K, C, tex, size, with_uvf, frame), wrap, with_scale)


def _reference_of(d, wrap, with_scale):
    image, T, grads = _model(d, wrap, with_scale, th.float64)
    image32, _, _ = _model(d, wrap, with_scale, th.float32, grads=False)
    noise = float(np.abs(image32.astype(np.float64) - image).max())
    return image, T, grads, noise, max(FWD_TOL, 4 * noise)


def _fused(d, dev, wrap, with_scale, want=GRADS, g_image=True, g_T=True, leaves=None):
    """composite_texture_fused on the device, gradients of `want` only -> image, T, {name: grad}.  leaves: {name: the device
    tensor to differentiate, as it is (its storage and offset)} in place of a fresh copy of d[name]."""
    t = {k: v.to(dev) for k, v in d.items() if isinstance(v, th.Tensor)}
    names = [k for k in want if with_scale or k != "face_scale"]
    lv = {k: (leaves[k].detach() if leaves and k in leaves else t[k].clone()).requires_grad_(True) for k in names}
    image, T = FG.composite_texture_fused(Fragments(t["face"], lv.get("bary", t["bary"]), None), t["faces"], lv.get("faces_opacity", t["faces_opacity"]),
                                          lv.get("vert_uvs", t["vert_uvs"]), lv.get("texture", t["texture"]),
                                          lv.get("face_scale", t["face_scale"]) if with_scale else None, uv_faces=t.get("uv_faces"), wrap=wrap)
    loss = 0
    if g_image is not False:
        loss = loss + (image * (t["g_image"] if g_image is True else g_image)).sum()
    if g_T is not False:
        loss = loss + (T * (t["g_T"] if g_T is True else g_T)).sum()
    grads = th.autograd.grad(loss, [lv[k] for k in names])
    return image.detach(), T.detach(), dict(zip(names, grads))


# K, C, texture (Ht, Wt), wrap, face_scale, uv_faces, size (shading_cases)
CASES = TEXTURE_CASES


@pytest.mark.parametrize("K,C,tex,wrap,with_scale,with_uvf,size", CASES,
                         ids=[f"K{c[0]}-C{c[1]}-{c[2][0]}x{c[2][1]}-{c[3]}-{'scale' if c[4] else 'no_scale'}-{'uvf' if c[5] else 'faces'}-{c[6]}" for c in CASES])
def test_caller_made_lists(hip_device, K, C, tex, wrap, with_scale, with_uvf, size):
    """(a) image, T and all five gradients against the float64 model.
    Measured on the MI355X over the 9 cases: image <= 2.1e-5 (32 x 48 texture; the model's float32 noise there 2.8e-5, bound
    1.1e-4), T <= 1.4e-7; rel_err of the gradients <= 1.0e-5 (faces_opacity), 1.2e-5 (vert_uvs), 7.7e-6 (texture), 6.8e-6
    (face_scale), 6.0e-6 (bary); 0.22 - 0.49 % of the used slots emptied near a texel-centre line."""
    d = _lists(K, C, tex, size, with_uvf)
    print(f"\nK {K} C {C} tex {tex} {wrap} {size} scale {with_scale} uv_faces {with_uvf}: {100 * d['removed']:.2f} % of the used slots near a texel-centre line")
    assert d["removed"] <= 0.02
    image_r, T_r, g_r, noise, bound = _reference(K, C, tex, size, with_uvf, wrap, with_scale)
    image, T, g = _fused(d, hip_device, wrap, with_scale)
    assert tuple(image.shape) == (B, C, H, W) and tuple(T.shape) == (B, 1, H, W)
    ei, eT = float(np.abs(image.cpu().numpy() - image_r).max()), float(np.abs(T.cpu().numpy() - T_r).max())
    print(f"  image {ei:.2e} (float32 noise of the model {noise:.2e}, bound {bound:.2e}; max |image| {np.abs(image_r).max():.3g}) T {eT:.2e}")
    assert ei <= bound and eT <= FWD_TOL
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
    """(b) each of the five alone equals the five together; a backward with only T's upstream equals one with a zero image
    upstream beside it, one with only the image's equals one with a zero upstream of T, and the two add up to the model's
    gradients.  Two evaluations of the same sums: sum_order_tol.  With only T's upstream everything but dL_dfaces_opacity is
    exactly 0."""
    K, C, tex, size, with_uvf, wrap = TEXTURE_ONLY_SOME
    d = _lists(K, C, tex, size, with_uvf)
    dev = hip_device
    _, _, g_all = _fused(d, dev, wrap, True)
    for k in GRADS:
        _, _, g = _fused(d, dev, wrap, True, want=(k,))
        e = rel_err(g[k].cpu().numpy(), g_all[k].cpu().numpy())
        print(f"\ndL_d{k} alone vs all five: {e:.2e}")
        assert list(g) == [k] and e <= sum_order_tol(k), (k, e)
    _, _, g_T = _fused(d, dev, wrap, True, g_image=False)
    _, _, g_T0 = _fused(d, dev, wrap, True, g_image=th.zeros_like(d["g_image"]).to(dev))
    _, _, g_I = _fused(d, dev, wrap, True, g_T=False)
    _, _, g_I0 = _fused(d, dev, wrap, True, g_T=th.zeros_like(d["g_T"]).to(dev))
    _, _, ref, _, _ = _reference(K, C, tex, size, with_uvf, wrap, True)
    for k in GRADS:
        e = rel_err(g_T[k].cpu().numpy(), g_T0[k].cpu().numpy())
        e2 = rel_err((g_T[k] + g_I[k]).cpu().numpy(), ref[k])
        e1 = rel_err(g_I[k].cpu().numpy(), g_I0[k].cpu().numpy())
        print(f"dL_d{k}: only grad_T vs zero grad_image {e:.2e}; only grad_image vs zero grad_T {e1:.2e}; the two summed vs the model {e2:.2e}")
        assert e <= sum_order_tol(k) and e1 <= sum_order_tol(k) and e2 <= GRAD_TOL, (k, e, e1, e2)
    for k in ("vert_uvs", "texture", "face_scale", "bary"):  # T depends on the opacities alone
        assert float(g_T[k].abs().max()) == 0.0, k


def test_ramp_identity_against_composite_fused(hip_device):
    """(c) without the model: the bilinear sample of the ramp tex[y, x] = a x + b y is the ramp, so with UVs inside
    [0.5/n, 1 - 0.5/n] and barycentrics inside the face composite_texture_fused equals composite_fused of the per-vertex
    attribute a (s Wt - 0.5) + b (t Ht - 0.5): image and T to the bound of (a), the opacity and scale gradients to GRAD_TOL.
    Measured on the MI355X: image 1.9e-6 (max |image| 12.3), T 0, dL_dfaces_opacity 9.8e-8, dL_dface_scale 2.6e-7."""
    dev = hip_device
    K, C, tex = 5, 3, (7, 13)
    Ht, Wt = tex
    d = dict(_lists(K, C, tex, "shared_keys", False))
    g = th.Generator().manual_seed(21)
    Pu = d["vert_uvs"].shape[0]
    lo = th.tensor([0.5 / Wt, 0.5 / Ht])
    d["vert_uvs"] = lo + th.rand(Pu, 2, generator=g) * (1 - 2 * lo)
    d["bary"] = th.rand(B, K, 2, H, W, generator=g) * 0.5
    ab = th.tensor([[0.7, -1.3], [0.25, 2.0], [-0.5, 0.4]])  # (a, b) per channel
    yy, xx = th.meshgrid(th.arange(Ht, dtype=th.float32), th.arange(Wt, dtype=th.float32), indexing="ij")
    d["texture"] = xx.unsqueeze(-1) * ab[:, 0] + yy.unsqueeze(-1) * ab[:, 1]
    attrs = ((d["vert_uvs"][:, :1].double() * Wt - 0.5) * ab[:, 0].double() + (d["vert_uvs"][:, 1:].double() * Ht - 0.5) * ab[:, 1].double()).float()
    image64, _, _ = _model(d, "clamp", True, th.float64, grads=False)
    image32, _, _ = _model(d, "clamp", True, th.float32, grads=False)
    noise = float(np.abs(image32.astype(np.float64) - image64).max())
    bound = max(FWD_TOL, 4 * noise)
    t = {k: v.to(dev) for k, v in d.items() if isinstance(v, th.Tensor)}
    out = {}
    for name in ("texture", "attrs"):
        op, sc = t["faces_opacity"].clone().requires_grad_(True), t["face_scale"].clone().requires_grad_(True)
        frag = Fragments(t["face"], t["bary"], None)
        if name == "texture":
            image, T = FG.composite_texture_fused(frag, t["faces"], op, t["vert_uvs"], t["texture"], sc, wrap="clamp")
        else:
            image, T = FG.composite_fused(frag, t["faces"], op, attrs.to(dev), face_scale=sc)
        g_op, g_sc = th.autograd.grad((image * t["g_image"]).sum() + (T * t["g_T"]).sum(), [op, sc])
        out[name] = (image.detach().cpu().numpy(), T.detach().cpu().numpy(), g_op.cpu().numpy(), g_sc.cpu().numpy())
    a, b = out["texture"], out["attrs"]
    ei, eT = float(np.abs(a[0] - b[0]).max()), float(np.abs(a[1] - b[1]).max())
    eo, es = rel_err(a[2], b[2]), rel_err(a[3], b[3])
    print(f"\nramp on the device, texture vs per-vertex attributes: image {ei:.2e} (bound {bound:.2e}, max |image| {np.abs(b[0]).max():.3g}) T {eT:.2e}; "
          f"dL_dfaces_opacity {eo:.2e} dL_dface_scale {es:.2e}")
    assert float(np.abs(b[0]).max()) > 1 and ei <= bound and eT <= FWD_TOL and eo <= GRAD_TOL and es <= GRAD_TOL


def test_rendered_tri_lists(hip_device):
    """(d) on the tri renderer's lists (fragment_grads): fused against composite_texture in float64 on the device -- the image
    and the two gradients that are continuous across texel cells (texture, opacity); verts.grad through frag.bary is finite and
    non-zero; and texture.grad sums, per channel, to sum over the fragments of w s g (the bilinear weights of a sample add to
    1): an exact check on the scatter that needs no model.
    Measured on the MI355X: image 1.1e-6, dL_dtexture 1.7e-7, dL_dfaces_opacity 3.0e-7, the per-channel sums 5.8e-9."""
    import dmesh_renderer_amd as dmr
    dev = hip_device
    K, Hs, Ws = 8, 80, 112
    d = scenes.layered_sheets(6, 8, 1, Hs, Ws, seed=3, opacity=(0.1, 0.4))
    t = {k: v.to(dev) for k, v in d.items()}
    r = dmr.TriRenderer(dmr.TriRenderSettings(Hs, Ws, t["bg"]), return_fragments=K, fragment_grads=True)
    verts = t["verts"].clone().requires_grad_(True)
    _, _, frag = r(*(verts if k == "verts" else t[k] for k in TRI_ARGS))
    assert frag.bary.requires_grad
    xy = t["verts"][:, :2]
    uvs = 0.1 + 0.8 * (xy - xy.min(0).values) / (xy.max(0).values - xy.min(0).values)
    gen = th.Generator().manual_seed(11)
    texture = th.randn(16, 16, 3, generator=gen).to(dev)
    gp = (th.rand(1, 3, Hs, Ws, generator=gen) + 0.5).to(dev)  # one sign: the sums below do not cancel
    tex_f, op_f = texture.clone().requires_grad_(True), t["faces_opacity"].clone().requires_grad_(True)
    image, _ = FG.composite_texture_fused(frag, t["faces"], op_f, uvs, tex_f, t["faces_intense"])
    g_tex, g_op, g_verts = th.autograd.grad((image * gp).sum(), [tex_f, op_f, verts])
    frag_c = dmr.Fragments(frag.pix_to_face, frag.bary.detach(), frag.count)
    tex_c, op_c = texture.double().requires_grad_(True), t["faces_opacity"].double().requires_grad_(True)
    image_c, _ = FG.composite_texture(frag_c, t["faces"], op_c, uvs.double(), tex_c, t["faces_intense"].double())
    r_tex, r_op = th.autograd.grad((image_c * gp.double()).sum(), [tex_c, op_c])
    image_32, _ = FG.composite_texture(frag_c, t["faces"], t["faces_opacity"], uvs, texture, t["faces_intense"])
    noise = float((image_32.double() - image_c.detach()).abs().max())
    bound = max(FWD_TOL, 4 * noise)
    ei = float((image.detach().double() - image_c.detach()).abs().max())
    et, eo = rel_err(g_tex.cpu().numpy(), r_tex.cpu().numpy()), rel_err(g_op.cpu().numpy(), r_op.cpu().numpy())
    print(f"\nrendered lists: image {ei:.2e} (float32 noise of the model {noise:.2e}, bound {bound:.2e}); dL_dtexture {et:.2e} "
          f"(max |ref| {float(r_tex.abs().max()):.3g}) dL_dfaces_opacity {eo:.2e} (max |ref| {float(r_op.abs().max()):.3g})")
    assert ei <= bound and et <= GRAD_TOL and eo <= GRAD_TOL
    assert bool(th.isfinite(g_verts).all()) and float(g_verts.abs().max()) > 0
    w = FG.blend_weights(frag_c, t["faces_opacity"].double())
    s = t["faces_intense"].double()[0][frag.pix_to_face.clamp(min=0).long()]
    expect = ((w * s).sum(1, keepdim=True) * gp.double()).sum((0, 2, 3)).cpu().numpy()
    got = g_tex.double().sum((0, 1)).cpu().numpy()
    e = rel_err(got, expect)
    print(f"texture.grad summed per channel {got} vs sum of w s g {expect}: {e:.2e}; max |verts.grad| {float(g_verts.abs().max()):.3g}")
    assert e <= GRAD_TOL


def test_graph_capture(hip_device):
    """(e) one forward + backward captured into a HIP graph and replayed: the replayed gradients are the eager ones."""
    K, C, tex, size, with_uvf = TEXTURE_GRAPH
    d = _lists(K, C, tex, size, with_uvf)
    dev = hip_device
    t = {k: v.to(dev) for k, v in d.items() if isinstance(v, th.Tensor)}
    lv = [t[k].clone().requires_grad_(True) for k in GRADS]

    def step():
        image, T = FG.composite_texture_fused(Fragments(t["face"], lv[4], None), t["faces"], lv[0], lv[1], lv[2], lv[3],
                                              uv_faces=t["uv_faces"], wrap="repeat")
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
# without a GPU that together they reach all 10 with both kinds of load, and that every case here meets check_inputs).
# ---------------------------------------------------------------------------
NO_TEX_GRAD = tuple(k for k in GRADS if k != "texture")


def check_inputs(d, ref, names=GRADS, signed=True):
    """What a case's inputs must give before anything is compared: at most 2 % of the used slots emptied near a texel-centre
    line, a non-zero reference for every compared gradient (an all-empty list cannot pass), and, under a one-signed upstream,
    opacity and scale gradients that no cancellation made small.  On a texture of one texel every sample is that texel: the UV
    and barycentric gradients are identically zero in the model (they are still compared), and only the others must be
    non-zero."""
    assert d["removed"] <= 0.02, d["removed"]
    g_r = ref[2]
    one_texel = d["texture"].shape[0] * d["texture"].shape[1] == 1
    for k in names:
        if k in g_r and not (one_texel and k in ("vert_uvs", "bary")):
            assert float(np.abs(g_r[k]).max()) > 0, k
    if not signed:
        assert float(np.abs(g_r["faces_opacity"]).max()) > 1 and float(np.abs(g_r["face_scale"]).max()) > 1


def _check(tag, d, ref, got, names=GRADS, signed=True):
    """image, T and the gradients `names` of `got` (device) against the float64 model `ref`, as test_caller_made_lists does."""
    check_inputs(d, ref, names, signed)
    image_r, T_r, g_r, noise, bound = ref
    image, T, g = got
    print(f"\n{tag}: {100 * d['removed']:.2f} % of the used slots near a texel-centre line")
    assert tuple(image.shape) == image_r.shape and tuple(T.shape) == T_r.shape
    ei, eT = float(np.abs(image.cpu().numpy() - image_r).max()), float(np.abs(T.cpu().numpy() - T_r).max())
    print(f"  image {ei:.2e} (float32 noise of the model {noise:.2e}, bound {bound:.2e}; max |image| {np.abs(image_r).max():.3g}) T {eT:.2e}")
    assert ei <= bound and eT <= FWD_TOL
    assert set(g) == {k for k in names if k in g_r}
    for k in g:
        x, r = g[k].cpu().numpy(), g_r[k]
        assert x.shape == r.shape and x.dtype == np.float32
        e = rel_err(x, r)
        print(f"  dL_d{k} {e:.2e} (max |ref| {np.abs(r).max():.3g})")
        assert e <= GRAD_TOL, (k, e)
    F = d["faces"].shape[0]
    empty = ((d["face"] < 0) | (d["face"] >= F))[:, :, None].expand(-1, -1, 2, -1, -1)
    if bool(empty.any()):  # empty slots: exact zeros in dL/dbary
        assert float(g["bary"].cpu()[empty].abs().max()) == 0.0


@functools.lru_cache(maxsize=None)
def _merge_lists(C, tex):
    """The merge-level lists of test_composite_fused_gpu._merge_lists (K = 6 on a 32 x 32 view, F = 5: stripes of period 2 .. 32
    along either axis in slots 0 .. 4, one face over every pixel in slot 5; opacities in (0.05, 0.4); one-signed upstreams), with
    UVs, a texture and uv_faces from the usual generator; slots near a texel-centre line emptied as everywhere."""
    B, H, W = MERGE_FRAME
    Ht, Wt = tex
    g = th.Generator().manual_seed(177 + C)
    py, px = th.meshgrid(th.arange(H), th.arange(W), indexing="ij")
    face = th.empty(B, MERGE_K, H, W, dtype=th.int32)
    for j in range(5):
        face[:, j] = th.where(py < 16, (px >> j) & 1, (py >> j) & 1).to(th.int32)
    face[:, 5] = 3
    bary = th.rand(B, MERGE_K, 2, H, W, generator=g) * 0.6 - 0.05
    faces = th.randint(0, MERGE_P, (MERGE_F, 3), generator=g, dtype=th.int32)
    uv_faces = th.randint(0, MERGE_P, (MERGE_F, 3), generator=g, dtype=th.int32)
    opacity = 0.05 + 0.35 * th.rand(MERGE_F, generator=g)
    assert bool(((opacity > 0.05) & (opacity < 0.4)).all())
    uvs = th.rand(MERGE_P, 2, generator=g) * 3 - 1
    texture = th.randn(Ht, Wt, C, generator=g)
    scale = th.rand(B, MERGE_F, generator=g) + 0.5
    g_image = th.rand(B, C, H, W, generator=g) + 0.5
    g_T = th.rand(B, 1, H, W, generator=g) + 0.5
    face, share = _off_the_lines(face, bary, uv_faces, uvs, Ht, Wt)
    return dict(face=face, bary=bary, faces=faces, uv_faces=uv_faces, faces_opacity=opacity, vert_uvs=uvs, texture=texture,
                face_scale=scale, g_image=g_image, g_T=g_T, removed=share)


@functools.lru_cache(maxsize=None)
def _merge_reference(C, tex, wrap):
    return _reference_of(_merge_lists(C, tex), wrap, True)


def new_cases():
    """(tag, lists, float64 reference, compared gradients, one-signed upstream) of every case below: what check_inputs must
    hold for."""
    for K, C, tex, wrap, with_scale, with_uvf, size in TEXTURE_MATRIX:
        yield (f"matrix K{K} C{C} {tex} {wrap} {size}", _lists(K, C, tex, size, with_uvf, NEW_FRAME),
               _reference(K, C, tex, size, with_uvf, wrap, with_scale, NEW_FRAME), GRADS, True)
    for K, C, tex, wrap, size in TEXTURE_NO_TEX_GRAD:
        yield (f"no texture gradient K{K} C{C} {tex} {wrap} {size}", _lists(K, C, tex, size, True, NEW_FRAME),
               _reference(K, C, tex, size, True, wrap, True, NEW_FRAME), NO_TEX_GRAD, True)
    for K, C, tex, wrap in TEXTURE_MISALIGNED:
        yield (f"misaligned K{K} C{C} {tex} {wrap}", _lists(K, C, tex, "table_overflow", True, NEW_FRAME),
               _reference(K, C, tex, "table_overflow", True, wrap, True, NEW_FRAME), GRADS, True)
    C, tex, wrap = TEXTURE_MERGE
    yield "merge levels", _merge_lists(C, tex), _merge_reference(C, tex, wrap), GRADS, False
    tex, wrap = TEXTURE_EDGE_FRAME
    for frame in EDGE_FRAMES:
        yield (f"frame {frame}", _lists(EDGE_FRAME_K, EDGE_FRAME_C, tex, "shared_keys", True, frame),
               _reference(EDGE_FRAME_K, EDGE_FRAME_C, tex, "shared_keys", True, wrap, True, frame), GRADS, True)


def _id(c):
    return "-".join(f"{x[0]}x{x[1]}" if isinstance(x, tuple) else (f"K{x}" if i == 0 else (f"C{x}" if i == 1 else str(x))) for i, x in enumerate(c))


@pytest.mark.parametrize("K,C,tex,wrap,with_scale,with_uvf,size", TEXTURE_MATRIX,
                         ids=[f"K{c[0]}-C{c[1]}-{c[2][0]}x{c[2][1]}-{c[3]}-{'scale' if c[4] else 'no_scale'}-{'uvf' if c[5] else 'faces'}-{c[6]}" for c in TEXTURE_MATRIX])
def test_instantiation_matrix(hip_device, K, C, tex, wrap, with_scale, with_uvf, size):
    """(f) the backward's KMAX = 16 kernels (1024 texel cells beside 32 KB of T_k and e_k), K == KMAX at 4, 8, 16 and 32, the
    first K of the next instantiation (9, 17), NCH = 8 with float4 loads, two scalar chunks (C = 5) and TEX_MAX_C, where the
    texel key t * nch + ch has its largest multiplier: image, T and all five gradients against the float64 model, on a 17 x 33
    view.
    Measured on the MI355X over the 7 cases: image <= 6.3e-6 (the model's float32 noise up to 9.0e-6, bound up to 3.6e-5; at most
    0.32 of a case's bound), T <= 1.8e-7; rel_err of the gradients <= 7.1e-6 (faces_opacity), 4.5e-6 (vert_uvs), 2.6e-6
    (texture), 6.1e-6 (face_scale), 3.8e-6 (bary); at most 0.47 % of the used slots emptied near a texel-centre line."""
    d = _lists(K, C, tex, size, with_uvf, NEW_FRAME)
    _check(f"K {K} C {C} tex {tex} {wrap} {size} scale {with_scale} uv_faces {with_uvf}", d,
           _reference(K, C, tex, size, with_uvf, wrap, with_scale, NEW_FRAME), _fused(d, hip_device, wrap, with_scale))


@pytest.mark.parametrize("K,C,tex,wrap,size", TEXTURE_NO_TEX_GRAD, ids=[_id(c) for c in TEXTURE_NO_TEX_GRAD])
def test_texture_gradient_not_wanted(hip_device, K, C, tex, wrap, size):
    """(g) the TEX = false instantiations (no texel table in LDS) at every KMAX, scalar and float4: the other four gradients
    against the float64 model.
    Measured on the MI355X over the 7 cases: image <= 5.9e-6 (bound up to 3.6e-5), T <= 1.5e-7; rel_err of the gradients <= 7.8e-6
    (faces_opacity), 5.9e-6 (vert_uvs), 7.5e-6 (face_scale), 4.8e-6 (bary); at most 0.52 % of the used slots emptied."""
    d = _lists(K, C, tex, size, True, NEW_FRAME)
    got = _fused(d, hip_device, wrap, True, want=NO_TEX_GRAD)
    assert list(got[2]) == list(NO_TEX_GRAD)
    _check(f"no texture gradient: K {K} C {C} tex {tex} {wrap} {size}", d, _reference(K, C, tex, size, True, wrap, True, NEW_FRAME), got,
           names=NO_TEX_GRAD)


@pytest.mark.parametrize("K,C,tex,wrap", TEXTURE_MISALIGNED, ids=[_id(c) for c in TEXTURE_MISALIGNED])
def test_misaligned_base(hip_device, K, C, tex, wrap):
    """(h) C % 4 == 0 with the texture one float into a larger buffer: the binding's .contiguous() keeps that pointer, so the
    scalar loads run (vec = 0) where the same values in a buffer of their own take the float4 loads.  Both against the float64
    model, and against each other (forward FWD_TOL; gradients: the same sums in another order, sum_order_tol).
    Measured on the MI355X over the 3 cases, either call against the model: image <= 3.5e-6 (bound up to 1.4e-5), T <= 1.8e-7,
    gradients <= 4.7e-6 (face_scale); misaligned against aligned: the forward bit-equal, dL_dfaces_opacity 3.5e-8, dL_dvert_uvs
    1.2e-7, dL_dtexture 7.6e-8, dL_dface_scale 3.0e-8, dL_dbary 0."""
    dev, size = hip_device, "table_overflow"
    d = _lists(K, C, tex, size, True, NEW_FRAME)
    ref = _reference(K, C, tex, size, True, wrap, True, NEW_FRAME)
    off, own = one_float_in(d["texture"].to(dev)), d["texture"].to(dev).clone()
    assert off.is_contiguous() and off.data_ptr() % 16 == 4 and own.data_ptr() % 16 == 0
    assert bool((off == own).all())
    got = _fused(d, dev, wrap, True, leaves={"texture": off})
    _check(f"K {K} C {C} tex {tex} {wrap} misaligned", d, ref, got)
    alg = _fused(d, dev, wrap, True, leaves={"texture": own})
    _check(f"K {K} C {C} tex {tex} {wrap} aligned", d, ref, alg)
    ei, eT = float((got[0] - alg[0]).abs().max()), float((got[1] - alg[1]).abs().max())
    print(f"misaligned vs aligned: image {ei:.2e} T {eT:.2e}; forward bit-equal: {bool(th.equal(got[0], alg[0]) and th.equal(got[1], alg[1]))}")
    assert ei <= FWD_TOL and eT <= FWD_TOL
    for k in GRADS:
        e = rel_err(got[2][k].cpu().numpy(), alg[2][k].cpu().numpy())
        print(f"  dL_d{k} misaligned vs aligned {e:.2e}")
        assert e <= sum_order_tol(k), (k, e)


def test_merge_levels(hip_device):
    """(i) shade_merge's four levels one at a time, and one face over a whole tile (_merge_lists), against the float64 model;
    the upstreams are one-signed, so the opacity and scale gradients (max |ref| > 1, asserted) cannot agree by cancellation.
    Measured on the MI355X: image 1.5e-6 (bound 1e-5), T 1.1e-7; dL_dfaces_opacity 6.1e-8 (max |ref| 2.4e3), dL_dvert_uvs 2.5e-7,
    dL_dtexture 2.5e-7, dL_dface_scale 3.4e-7 (max |ref| 167), dL_dbary 2.3e-6; 0.65 % of the used slots emptied."""
    C, tex, wrap = TEXTURE_MERGE
    d = _merge_lists(C, tex)
    _check(f"merge levels K {MERGE_K} C {C} tex {tex} {wrap}", d, _merge_reference(C, tex, wrap), _fused(d, hip_device, wrap, True), signed=False)


@pytest.mark.parametrize("frame", EDGE_FRAMES, ids=["x".join(map(str, f)) for f in EDGE_FRAMES])
def test_frames(hip_device, frame):
    """(j) a view of whole tiles only, and views of one pixel: one live lane per workgroup, the other 255 through every merge
    and barrier with key -1.
    Measured on the MI355X over both: image <= 5.0e-6 (bound 1.7e-5), T <= 5.5e-8; gradients <= 5.4e-6 (face_scale)."""
    K, C, size = EDGE_FRAME_K, EDGE_FRAME_C, "shared_keys"
    tex, wrap = TEXTURE_EDGE_FRAME
    d = _lists(K, C, tex, size, True, frame)
    _check(f"frame {frame} K {K} C {C}", d, _reference(K, C, tex, size, True, wrap, True, frame), _fused(d, hip_device, wrap, True))


def test_binding_refusals(hip_device):
    """The binding's own refusals, below fragments.py's: every case of shading_cases.binding_refusals("texture") raises a
    RuntimeError with the message the binding had before its list checks were merged (tests/golden/shading_refusals.json:
    copied from that source text and compared with a run of that binding over the same cases).
    One wrong argument per call, at one pixel: no call reaches a kernel."""
    import json
    import os
    import shading_cases as SC
    from dmesh_renderer_amd import _C
    golden = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shading_refusals.json")))["binding"]["texture"]
    cases = SC.binding_refusals("texture", hip_device)
    assert sorted({case for case, _, _ in cases}) == sorted(golden)
    for case, call, args in cases:
        with pytest.raises(RuntimeError) as e:
            getattr(_C, call)(*args)
        assert str(e.value) == golden[case], (case, call)
