"""The background terms of the CPU oracle (oracle/dmr_oracle.cpp), checked with a background that is not zero: util.BG.

With bg == 0 every one of them vanishes -- `T * bg` of the forwards, `bg_dot = bg . dL_dcolor` in every blended pair's
dL_dalpha of the backwards -- so the oracle, the yardstick of the GPU tests, is pinned here first, against the float64
autograd models of tests/tri_grad_ref.py and tests/tet_grad_ref.py (both composite over d["bg"]).  No GPU.
The brute-force forward tests of tests/test_oracle_cpu.py run over the same background.
"""
import numpy as np
import pytest

from dmesh_renderer_amd import scenes
from grad_cases import TRI_CASES, scene
from tet_grad_ref import TetGradRef
from tri_grad_ref import TriGradRef
from util import BG, rel_err, upstream_grads, with_bg

FWD_TOL = 1e-5
GRAD_TOL = 1e-4
BG_MATTERS = 0.5  # rel_err between the model's dL_dfaces_opacity over BG and over a zero background

_ZERO = (0.0, 0.0, 0.0)


def _grads_over(ref, bg, gc, gd):
    """ref.grads with the model's scene given the background `bg`."""
    kept = ref.d
    ref.d = with_bg(kept, bg)
    try:
        return ref.grads(gc, gd)
    finally:
        ref.d = kept


def _masked_upstream(ref, B, H, W):
    gc, gd = upstream_grads(B, H, W)
    m = ref.mask()
    return gc * m, gd * m


@pytest.mark.parametrize("case", ["one_view", "two_views_ragged"])
def test_tri_oracle_matches_float64_model_over_a_background(oracle, case):
    """The oracle's tri forward colour (kept pixels with blended pairs) and its gradients of verts_color, faces_opacity,
    verts_depth and faces_intense against the float64 model, over BG, the upstream gradients masked to the pixels the
    model keeps.  (dL_dverts is left out: the oracle's is the reference's formula, which is not the derivative -- SURVEY
    Q11, tests/test_tri_exact_grads_cpu.py asserts that the two disagree -- and the background does not enter it.)
    Measured (colour max-abs; rel_err of faces_opacity, largest of the other three; how far BG moves the model's
    dL_dfaces_opacity, rel_err against the zero-background one; kept pixels):
      one_view          4.8e-7; 1.8e-7, 8.3e-7; 1.44; 93 %
      two_views_ragged  3.5e-7; 1.4e-7, 7.1e-7; 1.88; 95 %"""
    L, n, B, H, W, rows = TRI_CASES[case]
    d = with_bg(scenes.layered_sheets(L, n, B, H, W, seed=7, opacity=(0.1, 0.5)))
    sc = oracle.scene_from_module_inputs(d, H, W)
    ocolor, _, ost = oracle.tri_forward(sc)
    ref = TriGradRef(d, H, W, ost)
    assert ref.kept_fraction >= 0.8, ref.kept_fraction
    gc, gd = _masked_upstream(ref, B, H, W)
    g, color, _ = ref.grads(gc, gd)
    g0, _, _ = _grads_over(ref, _ZERO, gc, gd)
    og = oracle.tri_backward(sc, ost, gc.numpy(), gd.numpy())
    ef = float(np.abs(ocolor[ref.view.numpy(), :, ref.py.numpy(), ref.px.numpy()] - color.numpy()).max())
    eg = {k: rel_err(og[k], g[k]) for k in ("verts_color", "faces_opacity", "verts_depth", "faces_intense")}
    moved = rel_err(g["faces_opacity"], g0["faces_opacity"])
    print(f"\ntri {case}: colour {ef:.2e}  " + "  ".join(f"dL_d{k} {e:.2e}" for k, e in eg.items())
          + f"  BG moves dL_dfaces_opacity by {moved:.2f}  kept {ref.kept_fraction:.3f}")
    assert moved >= BG_MATTERS, moved
    assert ef <= FWD_TOL, ef
    for k, e in eg.items():
        assert e <= GRAD_TOL, (k, e)
    # kept pixels without a blended pair show the bare background
    empty = ref.keep.clone()
    empty[ref.view, ref.py, ref.px] = False
    assert empty.any()
    px = ocolor.transpose(0, 2, 3, 1)[empty.numpy()]
    assert np.array_equal(px.view(np.uint32), np.broadcast_to(np.asarray(BG, np.float32), px.shape).copy().view(np.uint32))


_tet_cache = {}


def _tet(oracle, case):
    """The tet scene of a case over BG, the oracle's forward, the float64 model: once per case."""
    if case not in _tet_cache:
        d, B, H, W, seed = scene(case, bg=BG)
        sc = oracle.scene_from_module_inputs(d, H, W, seed=seed)
        ocolor, _, oactive, ost = oracle.tet_forward(sc)
        _tet_cache[case] = (d, B, H, W, sc, ocolor, oactive, ost, TetGradRef(d, H, W, ost))
    return _tet_cache[case]


# "opaque" is left out: the reference formula's opacity == 1 branch is itself 1e-3 away from the derivative there, with or
# without a background (tests/test_tet_full_grads_cpu.py)
@pytest.mark.parametrize("case", ["small", "jitter"])
def test_tet_oracle_matches_float64_model_over_a_background(oracle, case):
    """The oracle's tet forward colour (kept pixels) and both of its gradients against the float64 model, over BG, the
    upstream gradients masked to the pixels the model keeps.
    Measured (colour max-abs; rel_err of verts_color, faces_opacity; how far BG moves the model's dL_dfaces_opacity;
    kept pixels of the active ones):
      small   5.7e-7; 3.6e-7, 1.2e-7; 1.80; 97 %
      jitter  1.1e-6; 4.7e-7, 2.8e-7; 1.61; 96 %"""
    d, B, H, W, sc, ocolor, oactive, ost, ref = _tet(oracle, case)
    assert ref.n_active > 100 and ref.kept_fraction >= 0.8, (ref.n_active, ref.kept_fraction)
    gc, gd = _masked_upstream(ref, B, H, W)
    g, color, _ = ref.grads(gc, gd)
    g0, _, _ = _grads_over(ref, _ZERO, gc, gd)
    og = oracle.tet_backward(sc, ost, gc.numpy(), gd.numpy())
    HW = H * W
    ef = float(np.abs(ocolor.reshape(B, 3, HW)[ref.view.numpy(), :, (ref.pix % HW).numpy()] - color.numpy()).max())
    eg = {k: rel_err(og[k], g[k]) for k in ("verts_color", "faces_opacity")}
    moved = rel_err(g["faces_opacity"], g0["faces_opacity"])
    print(f"\ntet {case}: colour {ef:.2e}  " + "  ".join(f"dL_d{k} {e:.2e}" for k, e in eg.items())
          + f"  BG moves dL_dfaces_opacity by {moved:.2f}  kept {ref.kept_fraction:.3f}")
    assert moved >= BG_MATTERS, moved
    assert ef <= FWD_TOL, ef
    for k, e in eg.items():
        assert e <= GRAD_TOL, (k, e)


@pytest.mark.parametrize("case", ["small", "jitter"])
def test_inactive_tet_pixels_are_the_background(oracle, case):
    """A pixel whose march fails shows the bare background, bit for bit."""
    d, B, H, W, sc, ocolor, oactive, ost, ref = _tet(oracle, case)
    inactive = oactive < 0.5
    assert 0.1 < inactive.mean() < 0.9
    px = ocolor.transpose(0, 2, 3, 1)[inactive]
    assert np.array_equal(px.view(np.uint32), np.broadcast_to(np.asarray(BG, np.float32), px.shape).copy().view(np.uint32))
    assert not np.array_equal(ocolor.transpose(0, 2, 3, 1)[~inactive][0], np.asarray(BG, np.float32))
