"""Both renderers over a background that is not zero (util.BG = (0.9, -0.4, 1.7)).

With bg == 0 every background term of the kernels vanishes: `C + T * bg` of the tri forward (general path and the early
return of an empty tile), `C + fT * bg` / the bare `bg` of the tet forward, and `bg_dot = bg . dL_dcolor`, which enters
every blended pair's dL_dalpha in k_tri_backward_pix, k_tet_backward and k_tet_backward_seq (factor -T_final / (1 - alpha),
or -prev_T_final where alpha == 1).  Here they are checked
  * against the CPU oracle (pinned over the same background by tests/test_background_cpu.py): tests 1 and 3;
  * by the linearity of the image in the background, which does not lean on the oracle: test 2;
  * against the float64 models, for the opt-in gradient instantiations: test 4;
  * by the identities the README states, through the Modules: test 5;
  * under graph replay (the background is read at replay time) and through the binding's checks: tests 6 and 7.
Every test has a frame width no other test uses (widths = 4 mod 8), so its call 0 is the first call of its view
configuration.  Bounds: the project's FWD_TOL 1e-5, GRAD_TOL 1e-4 (rel_err: max-abs error over max(1, max-abs reference)),
SAME_TOL 1e-5 between two evaluations of the same sums; 1e-6 for the linearity (see LIN_TOL).  Every test prints what it
measured (pytest -s).  Measured on the MI355X, the three (two) calls alike:
  1. tri colour, depth, final_T bit-equal to the oracle's; dL_dfaces_opacity 7.2e-8 - 2.5e-7, the other gradients <= 1.3e-6;
  2. linearity 1.2e-7 (tri), 1.4e-7 (tet); the gradients but faces_opacity <= 4.5e-7 (tri), <= 5.0e-6 (tet, dL_dverts);
  3. tet colour <= 2.4e-7, depth <= 3.0e-7, dL_dverts_color <= 7.1e-7, dL_dfaces_opacity 9.5e-8 - 3.2e-7;
  4. dL_dfaces_opacity against the float64 models 2.3e-7 (tri), 1.2e-7 - 2.2e-7 (tet); dL_dverts 9.1e-7 / <= 6.1e-6, the
     matrices <= 7.8e-7 (tri), <= 2.7e-6 (tet), everything else <= 1.1e-6;
  5. colour + (1 - alpha) BG 1.4e-7, its gradients <= 2.2e-7, composite + T BG <= 2.4e-7;
  6. replayed gradients within 5.8e-7 of the eager step's;
and the background moves dL_dfaces_opacity by 1.2 - 3.7 times the tensor's own scale (rel_err against the zero-background one).
"""
import numpy as np
import pytest
import torch as th

from dmesh_renderer_amd import _through_inverse, scenes
from grad_cases import (CAM_TOL, FINT_TOL, MATS_TOL, SAME_TOL, TET_VERTS_TOL, TRI_CASES, TRI_VERTS_TOL, module_mats,
                        reference, scene, seq_state, setup)
from harness import TET_ARGS, TRI_ARGS, capture_replay, module_step, replay
from test_tri_parity_gpu import CASES as TRI_PARITY_CASES
from util import BG, SUM_ORDER_TOL, c_args, rel_err, upstream_grads, with_bg

pytestmark = pytest.mark.gpu

FWD_TOL = 1e-5
GRAD_TOL = 1e-4
# color_BG against color_0 + T * BG evaluated in float64: the kernel rounds T * bg and the sum to float32, values below 4
# (half an ulp each, 2.4e-7 at most, 3.6e-7 for the two with |T * bg| <= 1.7), plus one rounding where T is 1 - alpha
LIN_TOL = 1e-6
BG32 = np.asarray(BG, np.float32)
TRI_NAMES = ("verts", "verts_color", "faces_opacity", "verts_depth", "faces_intense")


def _is_bg(px):
    """px [..., 3] float32: every pixel is BG bit for bit."""
    return np.array_equal(np.ascontiguousarray(px).view(np.uint32), np.broadcast_to(BG32, px.shape).copy().view(np.uint32))


def _np(ts):
    return [x.cpu().numpy() for x in ts]


# ---- 1. tri, library against oracle -------------------------------------------------------------------------------------------
TRI_SCENES = {
    # name: (case of test_tri_parity_gpu.CASES, W, scale of verts)
    "C1_opaque": ("C1_opaque", 260, 1.0),       # early termination: T_final * bg of a stopped pixel
    "alpha_one": ("alpha_one", 276, 1.0),       # every 5th face of opacity exactly 1: the -prev_T_final * bg_dot branch
    "ragged": ("ragged", 332, 1.0),             # two views, partial tiles
    "dense": ("dense", 68, 1.0),                # several chunks per tile in the reverse walk
    "ragged_shrunk": ("ragged", 348, 0.4),      # empty tiles: the early-return path
}


def _tri_scene(name, bg=BG):
    case, W, scale = TRI_SCENES[name]
    L, n, B, H, _, op = TRI_PARITY_CASES[case]
    d = scenes.layered_sheets(L, n, B, H, W, seed=0, opacity=op)
    d["verts"] = d["verts"] * scale
    if case == "alpha_one":
        d["faces_opacity"][::5] = 1.0
    return with_bg(d, bg), B, H, W


@pytest.mark.parametrize("name", list(TRI_SCENES))
def test_tri_matches_oracle_over_a_background(oracle, hip_device, name):
    """Three calls: the first of the view configuration, a second default one (speculative binning, record regions laid out
    by the per-pixel kernel), an asynchronous one.  Lists bit-equal, colour / depth / final_T to FWD_TOL, the five gradients
    to GRAD_TOL; the pixels of empty tiles are BG bit for bit, their depth 1."""
    from dmesh_renderer_amd import _C
    d, B, H, W = _tri_scene(name)
    sc = oracle.scene_from_module_inputs(d, H, W)
    ocolor, odepth, ost = oracle.tri_forward(sc)
    gc, gd = upstream_grads(B, H, W)
    og = oracle.tri_backward(sc, ost, gc.numpy(), gd.numpy())
    oT = ost.get("final_T")
    if name == "C1_opaque":
        assert ((oT > 0) & (oT < 1e-4)).any(), "the scene must exercise early termination"
    if name == "alpha_one":
        assert (oT == 0).any(), "a pixel must end on a face of opacity 1"
    gx, gy = (W + 15) // 16, (H + 15) // 16
    r = ost.get("ranges").reshape(B, gy, gx, 2)
    empty = np.repeat(np.repeat(r[..., 1] <= r[..., 0], 16, axis=1), 16, axis=2)[:, :H, :W]  # [B,H,W]: pixels of empty tiles
    if name == "ragged_shrunk":
        assert empty.mean() > 0.5 and not empty.all(), "the scene must have empty tiles"
    args = c_args(d, hip_device)
    gcd, gdd = gc.to(hip_device), gd.to(hip_device)
    for call in range(3):
        _C.set_async(call == 2)
        try:
            out = _C.render_tris(*args, H, W)
            g = _C.render_tris_backward(*args, gcd, gdd, out[0], *out[3:7])
            th.cuda.synchronize()
        finally:
            _C.set_async(False)
        assert not _C.overflowed()
        R = ost.num_rendered
        assert out[0] == R if call < 2 else out[0] >= R  # (an asynchronous call reports its capacity)
        ex = lambda item, dt: _C.export(item, args, False, R, out[3:7], H, W, dt).cpu().numpy()
        np.testing.assert_array_equal(ex("ranges", th.int32).view(np.uint32), ost.get("ranges"))
        np.testing.assert_array_equal(ex("face_list", th.int32).view(np.uint32), ost.get("values"))
        np.testing.assert_array_equal(ex("n_contrib", th.int32).view(np.uint32), ost.get("n_contrib"))
        color, depth = out[1].cpu().numpy(), out[2].cpu().numpy()
        ec, ed = float(np.abs(color - ocolor).max()), float(np.abs(depth - odepth).max())
        et = float(np.abs(ex("final_T", th.float32) - oT).max())
        eg = {k: rel_err(got.cpu().numpy(), og[k]) for got, k in zip(g, TRI_NAMES)}
        print(f"\ntri {name} call {call}: colour {ec:.2e} depth {ed:.2e} final_T {et:.2e}  "
              + "  ".join(f"dL_d{k} {e:.2e}" for k, e in eg.items()))
        assert ec <= FWD_TOL and ed <= FWD_TOL and et <= FWD_TOL, (call, ec, ed, et)
        for k, e in eg.items():
            assert e <= GRAD_TOL, (call, k, e)
        if empty.any():
            assert _is_bg(color.transpose(0, 2, 3, 1)[empty]), call
            assert (depth[:, 0][empty] == 1.0).all(), call


# ---- 2. linearity in the background ---------------------------------------------------------------------------------------------
def test_tri_image_is_linear_in_the_background(hip_device):
    """color_BG == color_0 + final_T (x) BG, everything else unchanged; of the gradients only dL_dfaces_opacity moves."""
    from dmesh_renderer_amd import _C
    L, n, B, H, _, op = TRI_PARITY_CASES["ragged"]
    W = 364
    d = scenes.layered_sheets(L, n, B, H, W, seed=0, opacity=op)
    gc, gd = upstream_grads(B, H, W)
    gcd, gdd = gc.to(hip_device), gd.to(hip_device)
    res = []
    for bg in ((0.0, 0.0, 0.0), BG):
        args = c_args(with_bg(d, bg), hip_device)
        out = _C.render_tris(*args, H, W)
        g = _np(_C.render_tris_backward(*args, gcd, gdd, out[0], *out[3:7]))
        ex = lambda item, dt: _C.export(item, args, False, out[0], out[3:7], H, W, dt).cpu().numpy()
        res.append((out[0], out[1].cpu().numpy(), out[2].cpu().numpy(), ex("final_T", th.float32), ex("face_list", th.int32),
                    ex("ranges", th.int32), ex("n_contrib", th.int32), g))
    (R0, c0, z0, T0, fl0, rg0, nc0, g0), (R1, c1, z1, T1, fl1, rg1, nc1, g1) = res
    assert R0 == R1 and np.array_equal(fl0, fl1) and np.array_equal(rg0, rg1) and np.array_equal(nc0, nc1)
    assert np.array_equal(T0.view(np.uint32), T1.view(np.uint32)) and np.array_equal(z0.view(np.uint32), z1.view(np.uint32))
    assert 0.1 < (T1 == 1).mean() < 0.9 and (T1 < 0.5).any()
    want = c0.astype(np.float64) + T1.reshape(B, 1, H, W).astype(np.float64) * BG32.astype(np.float64).reshape(1, 3, 1, 1)
    e = float(np.abs(c1 - want).max())
    moved = rel_err(g1[2], g0[2])
    same = {k: rel_err(g1[i], g0[i]) for i, k in enumerate(TRI_NAMES) if k != "faces_opacity"}
    print(f"\ntri linearity: colour {e:.2e}  dL_dfaces_opacity moved by {moved:.2f}  " + "  ".join(f"dL_d{k} {v:.2e}" for k, v in same.items()))
    assert e <= LIN_TOL, e
    for k, v in same.items():  # (dL_dverts: its sums' order differs between two launches, util.SUM_ORDER_TOL)
        assert v <= (SUM_ORDER_TOL if k == "verts" else SAME_TOL), (k, v)
    assert moved > 0.5, moved


@pytest.mark.parametrize("seed", [0, 11])
def test_tet_image_is_linear_in_the_background(hip_device, seed):
    """color_BG == color_0 + (1 - alpha) (x) BG, inactive pixels BG bit for bit, everything else unchanged; of the four full
    gradients only dL_dfaces_opacity moves."""
    from dmesh_renderer_amd import _C
    d, B, H, W, _ = scene("two_views_ragged", W_extra=4 if seed == 0 else 20)
    gc, gd = upstream_grads(B, H, W)
    gcd, gdad = gc.to(hip_device), th.cat([gd, th.zeros_like(gd)], dim=1).to(hip_device)
    res = []
    for bg in ((0.0, 0.0, 0.0), BG):
        args = c_args(with_bg(d, bg), hip_device, tet=True)
        out = _C.render_tets(*args, H, W, seed, alpha=True)
        g = _np(_C.render_tets_backward(*args, gcd, gdad, *out[3:7], alpha=True, full_grads=True))
        ex = lambda item: _C.export(item, args, True, 0, out[3:7], H, W, th.int32).cpu().numpy()
        res.append((out[0].cpu().numpy(), out[1].cpu().numpy(), out[2].cpu().numpy(),
                    [ex(k) for k in ("first_face", "first_tet", "last_face", "last_tet", "n_contrib")], g))
    (c0, za0, a0, topo0, g0), (c1, za1, a1, topo1, g1) = res
    assert all(np.array_equal(x, y) for x, y in zip(topo0, topo1)) and np.array_equal(a0, a1)
    assert np.array_equal(za0.view(np.uint32), za1.view(np.uint32))  # depth and alpha
    inactive = a1 < 0.5
    assert 0.1 < inactive.mean() < 0.9
    assert _is_bg(c1.transpose(0, 2, 3, 1)[inactive]) and (za1[:, 1][inactive] == 0).all()
    T = 1.0 - za1[:, 1:].astype(np.float64)
    want = c0.astype(np.float64) + T * BG32.astype(np.float64).reshape(1, 3, 1, 1)
    e = float(np.abs(c1 - want).max())
    names = ("verts", "verts_color", "faces_opacity", "faces_intense")
    moved = rel_err(g1[2], g0[2])
    same = {k: rel_err(g1[i], g0[i]) for i, k in enumerate(names) if k != "faces_opacity"}
    print(f"\ntet linearity, seed {seed}: colour {e:.2e}  dL_dfaces_opacity moved by {moved:.2f}  "
          + "  ".join(f"dL_d{k} {v:.2e}" for k, v in same.items()))
    assert e <= LIN_TOL, e
    for k, v in same.items():
        assert v <= SAME_TOL, (k, v)
    assert moved > 0.5, moved


# ---- 3. tet, library against oracle ---------------------------------------------------------------------------------------------
def _malformed(W):
    """The scene of test_tet_parity_gpu.py::test_malformed_tets_stop_the_march_like_the_reference."""
    m, B, H = 5, 1, 112
    d = scenes.kuhn_tets(m, B, H, W, seed=3, opacity=(0.05, 0.4))
    tf = d["tet_faces"].clone()
    T = tf.shape[0]
    tf[3::11, 1] = tf[3::11, 0]           # the same face in two slots of a tet
    tf[5::13, 2] = tf[(7 + 5) % T, 0]     # a face of some other tet in the third slot
    d["tet_faces"] = tf.contiguous()
    return with_bg(d), B, H, W


TET_SCENES = {"small": 4, "two_views_ragged": 36, "opaque": 4, "malformed": 148}  # name: W_extra (malformed: W)


@pytest.mark.parametrize("name", list(TET_SCENES))
def test_tet_matches_oracle_over_a_background(oracle, hip_device, name):
    """Three calls: call 0 re-marches in the backward, call 1 runs on the forward's march sequence, call 2 is asynchronous.
    Topology and active bit-equal, colour and depth to FWD_TOL, both gradients to GRAD_TOL; pixels whose march fails -- in
    the malformed mesh also those that stop inside it -- are BG bit for bit."""
    from dmesh_renderer_amd import _C
    if name == "malformed":
        d, B, H, W = _malformed(TET_SCENES[name])
    else:
        d, B, H, W, _ = scene(name, W_extra=TET_SCENES[name], bg=BG)
    sc = oracle.scene_from_module_inputs(d, H, W)
    ocolor, odepth, oactive, ost = oracle.tet_forward(sc)
    gc, gd = upstream_grads(B, H, W)
    og = oracle.tet_backward(sc, ost, gc.numpy(), gd.numpy())
    inactive = oactive < 0.5
    assert 0.1 < inactive.mean() < 0.9
    if name == "malformed":
        assert (inactive & (ost.get("first_face").reshape(oactive.shape) >= 0)).any(), "marches must stop inside the mesh"
    args = c_args(d, hip_device, tet=True)
    gcd, gdd = gc.to(hip_device), gd.to(hip_device)
    for call in range(3):
        _C.set_async(call == 2)
        try:
            out = _C.render_tets(*args, H, W, 0)
            g = _C.render_tets_backward(*args, gcd, gdd, *out[3:7])
            th.cuda.synchronize()
        finally:
            _C.set_async(False)
        assert not _C.overflowed()
        longest, cap = seq_state(_C, args, out[3:7], H, W)
        assert longest == int(ost.get("n_contrib").max())
        if call < 2:
            assert (cap == 0) if call == 0 else (0 < longest <= cap), (call, longest, cap)
        ex = lambda item: _C.export(item, args, True, 0, out[3:7], H, W, th.int32).cpu().numpy()
        for item in ("first_face", "first_tet", "last_face", "last_tet"):
            np.testing.assert_array_equal(ex(item), ost.get(item), err_msg=item)
        np.testing.assert_array_equal(ex("n_contrib").view(np.uint32), ost.get("n_contrib"))
        np.testing.assert_array_equal(out[2].cpu().numpy(), oactive)
        color = out[0].cpu().numpy()
        ec, ed = float(np.abs(color - ocolor).max()), float(np.abs(out[1].cpu().numpy() - odepth).max())
        eg = {k: rel_err(got.cpu().numpy(), og[k]) for got, k in zip(g, ("verts_color", "faces_opacity"))}
        print(f"\ntet {name} call {call}: colour {ec:.2e} depth {ed:.2e}  " + "  ".join(f"dL_d{k} {e:.2e}" for k, e in eg.items()))
        assert ec <= FWD_TOL and ed <= FWD_TOL, (call, ec, ed)
        for k, e in eg.items():
            assert e <= GRAD_TOL, (call, k, e)
        assert _is_bg(color.transpose(0, 2, 3, 1)[inactive]), call


# ---- 4. the opt-in gradient instantiations against the float64 models -------------------------------------------------------------
def test_tri_exact_and_camera_grads_over_a_background(oracle, hip_device):
    """exact_grads=True and camera_grads=True (the other instantiations of k_tri_backward_pix's consumers), call 0 and call 1:
    every returned gradient against the float64 model -- faces_opacity, which the existing tests of these modes compare with
    the default path only, included."""
    from dmesh_renderer_amd import _C
    d, B, H, W, rows, gc, gd, rg = setup(oracle, "two_views_ragged", bg=BG, W_extra=4)
    args = c_args(d, hip_device)
    gcd, gdd = gc.to(hip_device), gd.to(hip_device)
    tol = {"verts": TRI_VERTS_TOL, "mv_mats": CAM_TOL, "proj_mats": CAM_TOL}
    for call in range(2):
        out = _C.render_tris(*args, H, W)
        for kw in ("exact_grads", "camera_grads"):
            g = _C.render_tris_backward(*args, gcd, gdd, out[0], *out[3:7], **{kw: True})
            got = dict(zip(TRI_NAMES, _np(g[:5])))
            if kw == "camera_grads":  # the gradients of the inverses of the transposed matrices -> of the row-major Module matrices
                got["mv_mats"] = _through_inverse(args[7], g[5]).transpose(1, 2).cpu().numpy()
                got["proj_mats"] = _through_inverse(args[8], g[6]).transpose(1, 2).cpu().numpy()
            eg = {k: rel_err(v, rg[k]) for k, v in got.items()}
            print(f"\ntri {kw} call {call}: " + "  ".join(f"dL_d{k} {e:.2e}" for k, e in eg.items()))
            for k, e in eg.items():
                assert e <= tol.get(k, GRAD_TOL), (call, kw, k, e)


@pytest.mark.parametrize("case", ["small", "jitter"])
def test_tet_full_and_camera_grads_over_a_background(oracle, hip_device, case):
    """full_grads=True and camera_grads=True, the FULL and CAM instantiations of k_tet_backward (call 0) and
    k_tet_backward_seq (call 1): every returned gradient against the float64 model."""
    from dmesh_renderer_amd import _C
    d, B, H, W, seed = scene(case, W_extra=36, bg=BG)
    ref, gc, gd, rg = reference(oracle, d, B, H, W, seed, camera=True)
    args = c_args(d, hip_device, tet=True)
    gcd, gdd = gc.to(hip_device), gd.to(hip_device)
    tol = {"verts": TET_VERTS_TOL, "faces_intense": FINT_TOL, "mv_mats": MATS_TOL, "proj_mats": MATS_TOL}
    for call in range(2):
        out = _C.render_tets(*args, H, W, seed)
        for kw in ("full_grads", "camera_grads"):
            g = _C.render_tets_backward(*args, gcd, gdd, *out[3:7], **{kw: True})
            th.cuda.synchronize()
            got = dict(zip(("verts", "verts_color", "faces_opacity", "faces_intense"), _np(g[:4])))
            if kw == "camera_grads":
                got["mv_mats"], got["proj_mats"] = module_mats(args, g)
            eg = {k: rel_err(v, rg[k]) for k, v in got.items()}
            print(f"\ntet {case} {kw} call {call}: " + "  ".join(f"dL_d{k} {e:.2e}" for k, e in eg.items())
                  + f"  kept {ref.kept_fraction:.3f}")
            for k, e in eg.items():
                assert e <= tol.get(k, GRAD_TOL), (call, kw, k, e)
        longest, cap = seq_state(_C, args, out[3:7], H, W)
        assert (cap == 0) if call == 0 else (0 < longest <= cap), (call, longest, cap)


# ---- 5. the advertised identities, through the Modules -----------------------------------------------------------------------------
def _identities(dmr, FG, make, t, names, up, K, dev):
    """make(bg, **kw) -> Module.  Renders over zeros and over BG (alpha and K fragments), and checks
    color_BG == color_0 + (1 - alpha_0) BG; the gradients of the loss on color_BG (the kernels' bg_dot) against those of the
    same loss on the torch-side composite of the first render (the alpha path only); composite(...) + T BG == color_BG."""
    tet = "tets" in t
    pos = TET_ARGS if tet else TRI_ARGS
    bg = th.tensor(BG, device=dev)
    own = {k: t[k].clone().requires_grad_(True) for k in names}
    outB = make(bg, return_alpha=True, return_fragments=K)(*(own.get(k, t[k]) for k in pos))
    colorB, depthB, alphaB, frag = outB[0], outB[1], outB[-2], outB[-1]
    th.autograd.backward([colorB, depthB], list(up))
    lv = {k: t[k].clone().requires_grad_(True) for k in names}
    out0 = make(th.zeros(3, device=dev), return_alpha=True)(*(lv.get(k, t[k]) for k in pos))
    color0, depth0, alpha0 = out0[0], out0[1], out0[-1]
    over = color0 + (1 - alpha0) * bg.view(1, 3, 1, 1)
    th.autograd.backward([over, depth0], list(up))
    assert th.equal(alphaB, alpha0) and th.equal(depthB, depth0)
    assert 0.1 < float((alpha0.detach() == 0).float().mean()) < 0.9 and float(alpha0.detach().max()) > 0.5
    want = color0.detach().double() + (1 - alpha0.detach().double()) * th.tensor(BG32, device=dev).double().view(1, 3, 1, 1)
    e = float((colorB.detach().double() - want).abs().max())
    eg = {k: rel_err(own[k].grad.cpu().numpy(), lv[k].grad.cpu().numpy()) for k in names}
    moved = rel_err(own["faces_opacity"].grad.cpu().numpy(), module_step(make(th.zeros(3, device=dev)), t, names, up)[1]["faces_opacity"].cpu().numpy())
    print(f"\n{'tet' if tet else 'tri'} Modules: colour over BG vs colour + (1 - alpha) BG {e:.2e}  "
          + "  ".join(f"dL_d{k} {v:.2e}" for k, v in eg.items()) + f"  (BG moves dL_dfaces_opacity by {moved:.2f})")
    assert e <= LIN_TOL, e
    for k, v in eg.items():
        assert v <= SAME_TOL, (k, v)
    assert moved > 0.5, moved
    within = (frag.count <= K)[:, None].expand_as(colorB)
    assert float(within.float().mean()) > 0.9
    comp, T = FG.composite(frag, t["faces"], t["faces_opacity"], t["verts_color"], face_scale=t["faces_intense"])
    ef = float(((comp + T * bg.view(1, 3, 1, 1)) - colorB.detach()).abs()[within].max())
    print(f"composite + T BG vs the Module's colour where count <= {K}: {ef:.2e}")
    assert ef <= FWD_TOL, ef


def test_tri_module_identities_over_a_background(hip_device):
    import dmesh_renderer_amd as dmr
    from dmesh_renderer_amd import fragments as FG
    L, n, B, H, W, _ = TRI_CASES["two_views_ragged"]
    W = W + 20
    d = scenes.layered_sheets(L, n, B, H, W, seed=7, opacity=(0.1, 0.5))
    t = {k: v.to(hip_device) for k, v in d.items()}
    up = [x.to(hip_device) for x in upstream_grads(B, H, W)]
    _identities(dmr, FG, lambda bg, **kw: dmr.TriRenderer(dmr.TriRenderSettings(H, W, bg), **kw), t,
                ("verts_color", "faces_opacity"), up, 8, hip_device)


def test_tet_module_identities_over_a_background(hip_device):
    """(two_views_ragged has no face of opacity 1: behind one the renderer keeps T = 1e-5 where composite gives 0, README.)"""
    import dmesh_renderer_amd as dmr
    from dmesh_renderer_amd import fragments as FG
    d, B, H, W, seed = scene("two_views_ragged", W_extra=52)
    assert float(d["faces_opacity"].max()) < 1
    t = {k: v.to(hip_device) for k, v in d.items()}
    up = [x.to(hip_device) for x in upstream_grads(B, H, W)]
    _identities(dmr, FG, lambda bg, **kw: dmr.TetRenderer(dmr.TetRenderSettings(H, W, bg, seed), **kw), t,
                ("verts_color", "faces_opacity"), up, 32, hip_device)


# ---- 6. graph replay reads the background at replay time ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["tri", "tet"])
def test_graph_replay_reads_the_background(hip_device, kind):
    """One step (forward + backward) captured with a static background tensor that holds zeros; BG copied into it; the replay
    must give the eager step over BG: images bit for bit, gradients to SAME_TOL."""
    from dmesh_renderer_amd import _C
    tet = kind == "tet"
    if tet:
        d, B, H, W, _ = scene("small", W_extra=68)
    else:
        L, n, B, H, W, _ = TRI_CASES["two_views_ragged"]
        W = W + 36
        d = scenes.layered_sheets(L, n, B, H, W, seed=2)
    args = c_args(d, hip_device, tet=tet)
    bg = args[0]
    assert bg.is_contiguous() and float(bg.abs().max()) == 0.0
    gcd, gdd = (x.to(hip_device) for x in upstream_grads(B, H, W))

    def step():
        if tet:
            out = _C.render_tets(*args, H, W, 0)
            return [out[0], out[1], *_C.render_tets_backward(*args, gcd, gdd, *out[3:7])]
        out = _C.render_tris(*args, H, W)
        return [out[1], out[2], *_C.render_tris_backward(*args, gcd, gdd, out[0], *out[3:7])]

    graph, captured, black = capture_replay(step)
    bg.copy_(th.tensor(BG))
    replay(graph)
    th.cuda.synchronize()
    eager = [x.clone() for x in step()]
    th.cuda.synchronize()
    assert th.equal(captured[0], eager[0]) and th.equal(captured[1], eager[1])
    assert not th.equal(captured[0], black[0])
    eg = [rel_err(a.cpu().numpy(), b_.cpu().numpy()) for a, b_ in zip(captured[2:], eager[2:])]
    fo = 1 if tet else 2
    moved = rel_err(captured[2 + fo].cpu().numpy(), black[2 + fo].cpu().numpy())
    print(f"\n{kind} replay over BG vs eager: gradients " + " ".join(f"{e:.2e}" for e in eg) + f"  (BG moves dL_dfaces_opacity by {moved:.2f})")
    for e in eg:
        assert e <= SAME_TOL, eg
    assert moved > 0.5, moved


# ---- 7. the binding's checks and layouts of the background --------------------------------------------------------------------------
def test_background_binding_checks(hip_device):
    from dmesh_renderer_amd import _C
    dev = hip_device
    H, W = 32, 36
    tri = c_args(with_bg(scenes.layered_sheets(2, 4, 1, H, W)), dev)
    tet = c_args(with_bg(scenes.kuhn_tets(2, 1, H, W)), dev, tet=True)
    calls = ((lambda a: _C.render_tris(*a, H, W)[1:3], tri), (lambda a: _C.render_tets(*a, H, W, 0)[0:3], tet))
    for render, args in calls:
        with pytest.raises(RuntimeError, match="all tensors must be on"):
            render([args[0].cpu()] + args[1:])
        with pytest.raises(RuntimeError, match="background must have 3 channels"):
            render([args[0][:2]] + args[1:])
        want = render(args)
        assert (want[0][:, :, 0, 0].cpu() == th.tensor(BG)).all()  # a corner pixel: nothing there but the background
        strided = th.tensor([0.9, 9, -0.4, 9, 1.7, 9], device=dev)[::2]
        assert not strided.is_contiguous()
        for bg in (strided, args[0].reshape(1, 3)):
            got = render([bg] + args[1:])
            assert all(th.equal(a, b_) for a, b_ in zip(got, want))
