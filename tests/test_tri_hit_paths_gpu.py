"""tri renderer: all three instantiations of k_tri_backward_hits (TRI_GRAD_REF, TRI_GRAD_EXACT, TRI_GRAD_CAMERA), k_tri_backward_pix
and k_tri_camera_reduce against the float64 model of tests/tri_grad_ref.py on the edge scenes of tests/tri_hit_cases.py -- the
paths the three scenes of grad_cases.TRI_CASES never take (tests/test_tri_hit_paths_cpu.py asserts, without a GPU, that each case
does take them, and that the model agrees with the CPU oracle there on the four gradients the reference computes exactly):
  crowded_*  tens of rounds per tile (the nine ray moments, camT and L.dray carried across rounds and DPP rows) and thousands of
             distinct vertex rows for a table of 560 (tab_find3 gives -1: the exact rows leave through direct atomics, in the
             product build, exact and camera variant alike);
  opaque_*   pixels that stop at T < T_EPS and faces of opacity exactly 1 (alpha == 1 with prev_T_final in k_tri_backward_pix),
             under faces that cover dozens of tiles: dL_dverts and the matrices there, not only dL_dfaces_opacity;
  wide*      529 tiles per view: every thread row of k_tri_camera_reduce<32> runs its four-loads-in-flight loop, and the two loops
             split the tiles unevenly (529 = 4 * 128 + 17);
  tet_wide*  289 tiles per view, the same for k_tri_camera_reduce<64> behind both tet backward kernels.
Every case runs two calls (the first backward of its view configuration, with record regions from k_scan_hits, and a later
one); each call runs the default, the exact_grads=True and the camera_grads=True backward on one forward.

Bars (the project's own, tests/grad_cases.py and tests/util.py): forward 1e-5 on the kept pixels with pairs; dL_dverts of the
exact and camera levels TRI_VERTS_TOL = 1e-4; dL_dmv_mats, dL_dproj_mats CAM_TOL = 1e-3 (tet: MATS_TOL); verts_color,
faces_opacity, verts_depth, faces_intense of all three levels against the model 1e-4, the opt-in levels' within SAME_TOL = 1e-5
of the default call's; the translation identity ID_TOL = 1e-4 (B == 1); the second call within sum_order_tol(name) of the first.
rel_err divides by max(1, max|ref|): every comparison also asserts max|ref| >= 1 (_rel), so the bars are relative; the crowded
cases' upstream gradients are scaled by a power of two chosen from the model alone for that (tri_hit_cases.Ref).

MEASURED on the MI355X, the worse of the two calls (every comparison prints its figure, pytest -s).  dL_dverts: exact / camera
level against the model; mats: dL_dmv_mats / dL_dproj_mats; id: the translation identity; four: the worst of the four
exactly-computed gradients over the three levels against the model; same: those of the opt-in levels against the default
call's; repeat: call 1 against call 0, the worst tensor of the three levels (matrices included):
  case                dL_dverts          mats               id      four    same    repeat
  crowded_one_tile    2.3e-6 / 2.2e-6    2.5e-6 / 3.2e-6    2.6e-8  2.7e-6  2.1e-7  7.9e-7
  crowded_four_tiles  2.0e-6 / 1.9e-6    9.1e-7 / 1.1e-6    2.9e-8  1.4e-6  1.6e-7  5.3e-7
  crowded_two_views   4.7e-7 / 4.7e-7    1.4e-6 / 1.1e-6    -       6.6e-7  1.8e-7  5.9e-7
  opaque_deep         5.8e-7 / 6.3e-7    3.2e-7 / 2.4e-7    1.9e-8  5.6e-7  2.8e-7  5.4e-7
  opaque_two_views    2.6e-7 / 2.8e-7    1.9e-7 / 1.6e-7    -       3.9e-7  1.2e-7  1.6e-7
  wide                1.3e-6 / 1.3e-6    6.5e-7 / 2.6e-7    7.8e-9  1.3e-6  2.3e-7  7.3e-7
  wide_two_views      9.5e-7 / 9.1e-7    7.8e-7 / 1.6e-7    -       7.1e-7  3.1e-7  5.8e-7
forward: colour <= 6.3e-7, depth <= 1.1e-6.  (The default level's dL_dverts is the reference renderer's formula, another
function: 0.58-0.98 of the model's largest entry away; printed, not asserted.)  No case exceeded a bar: these tests changed no
kernel.  The 37 tests take 7.4 s together, 2.4 s the slowest (wide_two_views: its float64 model), shared by the case's five tests.

The non-finite branch of k_tri_backward_hits (chk != 0) is reached by none of these scenes: every input is finite, no kept pair
has denom == 0 (the forward skips those, HIT_SKIPPED), and a face of opacity 1 leaves T == 0 < T_EPS, so it is its pixel's last
contributor and k_tri_backward_pix never multiplies by its 1 / (1 - alpha).
"""
import numpy as np
import pytest
import torch as th

import tri_hit_cases as HC
from grad_cases import CAM_TOL, ID_TOL, MATS_TOL, SAME_TOL, TRI_VERTS_TOL, module_mats, seq_state
from test_fragment_grads_gpu import _module_mats, _rel
from test_tet_camera_grads_gpu import _identity as _tet_identity
from test_tri_exact_grads_gpu import _identity
from util import c_args, rel_err, sum_order_tol

pytestmark = pytest.mark.gpu

FWD_TOL = 1e-5
MODEL_TOL = 1e-4   # the four exactly-computed gradients against the model
LEVELS = (("default", {}), ("exact", {"exact_grads": True}), ("camera", {"camera_grads": True}))

_runs = {}


def _run(oracle, hip_device, case):
    """Both calls of a case, once for the module: per call the forward and the three levels' gradients as numpy arrays, the
    camera level's Module-matrix gradients, and whether the call overflowed."""
    if case in _runs:
        return _runs[case]
    from dmesh_renderer_amd import _C
    r = HC.reference(oracle, case)
    args = c_args(r.d, hip_device)
    gcd, gdd = r.gc.to(hip_device), r.gd.to(hip_device)
    _C.overflowed()   # (reset: the flag is the process's)
    calls = []
    for call in range(2):
        out = _C.render_tris(*args, r.H, r.W)
        g = {}
        # call 0 camera level first: the first backward of the view configuration is the one whose record regions k_scan_hits lays
        # out (the default level's first backward is test_tri_parity_gpu's business); call 1 in the table's order
        for name, kw in (LEVELS[::-1] if call == 0 else LEVELS):
            g[name] = _C.render_tris_backward(*args, gcd, gdd, out[0], *out[3:7], **kw)
        th.cuda.synchronize()
        overflowed = bool(_C.overflowed())
        mats = _module_mats(args, g["camera"])
        calls.append({
            "R": int(out[0]), "color": out[1].cpu().numpy(), "depth": out[2].cpu().numpy(), "overflowed": overflowed,
            "g": {name: [x.cpu().numpy() for x in v] for name, v in g.items()}, "mv_mats": mats[0], "proj_mats": mats[1],
        })
    _runs[case] = (r, calls)
    return _runs[case]


@pytest.mark.parametrize("case", list(HC.CASES))
def test_forward_matches_model_and_nothing_overflows(oracle, hip_device, case):
    r, calls = _run(oracle, hip_device, case)
    m = r.model
    v, y, x = m.view.numpy(), m.py.numpy(), m.px.numpy()
    for call, c in enumerate(calls):
        assert not c["overflowed"], call
        assert c["R"] == r.st.num_rendered
        ec = float(np.abs(c["color"][v, :, y, x] - r.model_color.numpy()).max())
        ed = float(np.abs(c["depth"][v, 0, y, x] - r.model_depth.numpy()).max())
        print(f"\n{case} call {call}: forward colour {ec:.2e} depth {ed:.2e}  ({len(v)} kept pixels with pairs, kept {m.kept_fraction:.3f})")
        assert ec <= FWD_TOL and ed <= FWD_TOL, (call, ec, ed)


@pytest.mark.parametrize("case", list(HC.CASES))
def test_exact_and_camera_verts_match_model(oracle, hip_device, case):
    """dL_dverts of the exact and the camera level against the float64 model, both calls."""
    r, calls = _run(oracle, hip_device, case)
    for call, c in enumerate(calls):
        ev = _rel(c["g"]["exact"][0], r.grads["verts"], "verts")
        ek = _rel(c["g"]["camera"][0], r.grads["verts"], "verts")
        print(f"\n{case} call {call}: dL_dverts exact {ev:.2e} camera {ek:.2e}  (the default's, another formula: "
              f"{rel_err(c['g']['default'][0], r.grads['verts']):.2e}; max|model| {np.abs(r.grads['verts']).max():.3g}, factor {r.factor:g})")
        assert ev <= TRI_VERTS_TOL and ek <= TRI_VERTS_TOL, (call, ev, ek)


@pytest.mark.parametrize("case", list(HC.CASES))
def test_camera_matrices_match_model(oracle, hip_device, case):
    """The camera level's dL/dinv_mv, dL/dinv_proj through the chain the autograd Function applies, against the model's dL_dmv_mats
    and dL_dproj_mats; B == 1: the translation identity."""
    r, calls = _run(oracle, hip_device, case)
    for call, c in enumerate(calls):
        gk = c["g"]["camera"]
        assert len(gk) == 7 and gk[5].shape == (r.B, 4, 4) and gk[6].shape == (r.B, 4, 4)
        em = _rel(c["mv_mats"], r.grads["mv_mats"], "mv_mats")
        ep = _rel(c["proj_mats"], r.grads["proj_mats"], "proj_mats")
        print(f"\n{case} call {call}: dL_dmv_mats {em:.2e}  dL_dproj_mats {ep:.2e}  "
              f"(|dL_dmv| {np.abs(r.grads['mv_mats']).max():.3g}, |dL_dproj| {np.abs(r.grads['proj_mats']).max():.3g})")
        assert em <= CAM_TOL and ep <= CAM_TOL, (call, em, ep)
        if r.B == 1:   # the ray origin and the three vertices enter (u, v) only as differences
            e = _identity(gk[0], gk[5])
            print(f"{case} call {call}: translation identity {e:.2e}")
            assert e <= ID_TOL, (call, e)


@pytest.mark.parametrize("case", list(HC.CASES))
def test_exactly_computed_gradients_match_model_at_all_levels(oracle, hip_device, case):
    """verts_color, faces_opacity, verts_depth, faces_intense: every level against the float64 model, and the opt-in levels
    against the default call's."""
    r, calls = _run(oracle, hip_device, case)
    for call, c in enumerate(calls):
        for level, _ in LEVELS:
            g = c["g"][level]
            assert len(g) == (7 if level == "camera" else 5)
            errs = {k: _rel(g[i], r.grads[k], k) for i, k in enumerate(HC.GRAD_KEYS) if i > 0}
            print(f"\n{case} call {call} {level}: against the model " + "  ".join(f"{k} {e:.2e}" for k, e in errs.items()))
            assert max(errs.values()) <= MODEL_TOL, (call, level, errs)
            if level != "default":
                same = {k: _rel(g[i], c["g"]["default"][i], k) for i, k in enumerate(HC.GRAD_KEYS) if i > 0}
                print(f"{case} call {call} {level}: against the default call " + "  ".join(f"{k} {e:.2e}" for k, e in same.items()))
                assert max(same.values()) <= SAME_TOL, (call, level, same)


@pytest.mark.parametrize("case", list(HC.CASES))
def test_later_call_repeats_the_first(oracle, hip_device, case):
    """The second backward of the view configuration (placed record regions) against the first (scanned ones): the same sums in
    another order."""
    r, calls = _run(oracle, hip_device, case)
    for level, _ in LEVELS:
        a, b_ = calls[0]["g"][level], calls[1]["g"][level]
        errs = {k: _rel(b_[i], a[i], k) for i, k in enumerate(HC.GRAD_KEYS)}
        tols = {k: sum_order_tol(k) for k in HC.GRAD_KEYS}
        if level == "camera":   # the matrices: sums of the same pairs' ray terms as dL_dverts, through the same chain
            for k in ("mv_mats", "proj_mats"):
                errs[k], tols[k] = _rel(calls[1][k], calls[0][k], k), sum_order_tol("verts")
        print(f"\n{case} {level}: call 1 against call 0 " + "  ".join(f"{k} {e:.2e}" for k, e in errs.items()))
        for k, e in errs.items():
            assert e <= tols[k], (level, k, e)


@pytest.mark.parametrize("case", list(HC.TET_WIDE))
def test_tet_camera_grads_wide_frame(oracle, hip_device, case):
    """289 tiles per view: every thread row of k_tri_camera_reduce<64> runs the four-loads-in-flight loop.  The first call of the
    view configuration (the re-marching k_tet_backward) and the second (k_tet_backward_seq) with camera gradients against
    TetCameraGradRef, as test_tet_camera_grads_gpu.test_camera_grads_match_float64_reference does for frames of at most 216.
    Measured on the MI355X (rel_err dL_dmv / dL_dproj, translation identity; call 0 and call 1; kept pixels):
      tet_wide            9.5e-7 / 3.2e-7, 2.7e-8;  5.1e-7 / 2.7e-7, 3.2e-8  (97.1 %)
      tet_wide_two_views  9.0e-7 / 9.3e-7, 6.6e-8;  3.5e-7 / 1.1e-6, 4.1e-8  (96.5 %)"""
    from dmesh_renderer_amd import _C
    d, B, H, W, seed, ref, gc, gd, rg = HC.tet_reference(oracle, case)
    args = c_args(d, hip_device, tet=True)
    gcd, gdd = gc.to(hip_device), gd.to(hip_device)
    cams = []
    for call in range(2):
        out = _C.render_tets(*args, H, W, seed)
        gk = _C.render_tets_backward(*args, gcd, gdd, *out[3:7], camera_grads=True)
        gf = _C.render_tets_backward(*args, gcd, gdd, *out[3:7], full_grads=True)
        th.cuda.synchronize()
        longest, cap = seq_state(_C, args, out[3:7], H, W)
        assert (cap == 0) if call == 0 else (0 < longest <= cap), (call, longest, cap)
        assert len(gk) == 8 and all(x.shape == (B, 4, 4) for x in gk[4:])
        g_mv, g_proj = module_mats(args, gk)
        em, ep = _rel(g_mv, rg["mv_mats"], "mv_mats"), _rel(g_proj, rg["proj_mats"], "proj_mats")
        ei = _tet_identity(d, gk)
        print(f"\n{case} call {call}: dL_dmv {em:.2e}  dL_dproj {ep:.2e}  identity {ei:.2e}  kept {ref.kept_fraction:.3f}")
        assert em <= MATS_TOL and ep <= MATS_TOL, (call, em, ep)
        assert ei <= ID_TOL, (call, ei)
        for a, b_ in zip(gk[:4], gf):
            assert rel_err(a.cpu().numpy(), b_.cpu().numpy()) <= SAME_TOL
        cams.append([x.cpu().numpy() for x in gk])
    for a, b_ in zip(cams[0], cams[1]):  # re-march vs sequence kernel
        assert rel_err(a, b_) <= SAME_TOL
