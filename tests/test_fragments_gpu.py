"""The tri renderer's per-pixel fragment lists on the GPU (DMR_FLAG_TRI_FRAGMENTS; `fragments=K` of the binding;
return_fragments=K of TriRenderer; helpers in dmesh_renderer_amd/fragments.py) against the CPU oracle's forward state and
against the float64 model of tests/tri_grad_ref.py (checks: tests/fragments_ref.py).

Bounds (the project's own): forward quantities 1e-5 absolute (FWD_TOL), gradients rel_err <= 1e-4 (GRAD_TOL); face ids,
counts and everything the option must not move: exact.  Every case prints what it measured (pytest -s).
"""
import numpy as np
import pytest
import torch as th

import fragments_ref as FR
from dmesh_renderer_amd import scenes
from grad_cases import TRI_CASES
from harness import TRI_ARGS, capture_replay, replay
from tri_grad_ref import TriGradRef
from util import c_args, rel_err, sum_order_tol, upstream_grads

pytestmark = pytest.mark.gpu

FWD_TOL = FR.FWD_TOL
GRAD_TOL = 1e-4
K = 8
TRI_NAMES = ("verts", "verts_color", "faces_opacity", "verts_depth", "faces_intense")


def _frag(out):
    """face, bary, count of a render_tris(fragments=K) tuple as numpy."""
    assert len(out) == 10
    face, bary, count = (t.cpu().numpy() for t in out[7:10])
    assert face.dtype == np.int32 and bary.dtype == np.float32 and count.dtype == np.int32
    return face, bary, count


def _oracle(oracle, d, H, W, rows=(0, 0)):
    sc = oracle.scene_from_module_inputs(d, H, W, rows=rows)
    return (sc,) + tuple(oracle.tri_forward(sc))


def _check_state(oracle, dev, d, B, H, W, rows, tag, k=K, calls=2):
    """Check (a) on call 0 and call 1 of the view configuration -> (oracle scene, state, the last call's fragments)."""
    from dmesh_renderer_amd import _C
    sc, ocolor, odepth, ost = _oracle(oracle, d, H, W, rows)
    args = c_args(d, dev)
    for call in range(calls):
        out = _C.render_tris(*args, H, W, rows=rows, fragments=k)
        face, bary, count = _frag(out)
        assert face.shape == (B, k, H, W) and bary.shape == (B, k, 2, H, W) and count.shape == (B, H, W)
        assert int(count.max()) <= k, "K must cover the scene's deepest pixel"
        FR.check_lists(sc, ost, face, bary, count, rows)
        FR.check_composite(sc, ost, ocolor, odepth, face, bary, count, rows, tag=f"{tag} call {call}")
    return sc, ost, (face, bary, count)


@pytest.mark.parametrize("case", list(TRI_CASES))
def test_fragments_match_oracle_and_model(oracle, hip_device, case):
    """(a) against the oracle's state and (b) against the independent float64 model, on the cases and seed for which
    tests/test_tri_exact_grads_gpu.py demands the model's kept fraction (grad_cases.setup): the same bound here."""
    from dmesh_renderer_amd import _C
    L, n, B, H, W, rows = TRI_CASES[case]
    d = scenes.layered_sheets(L, n, B, H, W, seed=7, opacity=(0.1, 0.5))
    _check_state(oracle, hip_device, d, B, H, W, rows, case)
    _, _, _, ost_full = _oracle(oracle, d, H, W)
    ref = TriGradRef(d, H, W, ost_full)
    assert ref.kept_fraction >= 0.8, ref.kept_fraction
    args = c_args(d, hip_device)
    for call in range(2):
        face, bary, count = _frag(_C.render_tris(*args, H, W, rows=rows, fragments=K))
        FR.check_model(ref, d, face, bary, count, rows)


def _deep_scene(B=1, H=80, W=112):
    return scenes.layered_sheets(6, 8, B, H, W, seed=3, opacity=(0.1, 0.4)), B, H, W


def test_truncation(oracle, hip_device):
    """fragments=2 on a scene with deeper pixels: the first two slots of the K = 8 call, the same count."""
    from dmesh_renderer_amd import _C
    d, B, H, W = _deep_scene()
    args = c_args(d, hip_device)
    for call in range(2):
        f8, b8, c8 = _frag(_C.render_tris(*args, H, W, fragments=8))
        f2, b2, c2 = _frag(_C.render_tris(*args, H, W, fragments=2))
        assert int(c8.max()) <= 8 and (c8 > 2).any()
        assert np.array_equal(c2, c8)
        assert np.array_equal(f2, f8[:, :2]) and np.array_equal(b2.view(np.uint32), b8[:, :2].view(np.uint32))


def test_nothing_else_moves(hip_device):
    """Colour, depth, alpha and the scratch tensors' sizes with and without `fragments`; the backward on either forward.
    The tri backward does not repeat bit for bit even on ONE forward state (record claim order, float atomics across tiles:
    tests/test_fullsize_gpu.py asserts "backward twice from one forward" to sum_order_tol for that reason), so "the same
    gradients" is stated as: everything the backward reads of the forward state is bit-identical, and the gradients agree
    within that same sum_order_tol.  Whether they came out bit-identical is printed."""
    from dmesh_renderer_amd import _C
    d, B, H, W = _deep_scene(B=2, W=128)
    args = c_args(d, hip_device)
    gc, gd = upstream_grads(B, H, W)
    gc, gd = gc.to(hip_device), gd.to(hip_device)
    # The binning buffer is sized by a call's index in its view configuration (exact R, then the estimate, then the placement's
    # capacity), whatever the option: two calls compare at the same index only once the configuration is warm, both placed.
    for _ in range(2):
        _C.render_tris(*args, H, W)
    for call in range(2):
        for akw in ({}, {"alpha": True}):
            o0 = _C.render_tris(*args, H, W, **akw)
            o1 = _C.render_tris(*args, H, W, fragments=4, **akw)
            assert len(o0) == 7 and len(o1) == 10 and o0[0] == o1[0]
            assert th.equal(o0[1], o1[1]) and th.equal(o0[2], o1[2]), "colour / depth (/ alpha) must not change with the option"
            for i, (a, b) in enumerate(zip(o0[3:7], o1[3:7])):
                assert a.dtype == b.dtype and a.shape == b.shape, (call, i, a.shape, b.shape)
        o0 = _C.render_tris(*args, H, W)
        o1 = _C.render_tris(*args, H, W, fragments=4)
        for name in ("ranges", "face_list", "n_contrib", "final_T", "final_prev_T", "tile_hits"):  # what the backward reads
            x0, x1 = (_C.export(name, args, False, o[0], o[3:7], H, W, th.int32) for o in (o0, o1))
            assert th.equal(x0, x1), name
        g0 = _C.render_tris_backward(*args, gc, gd, o0[0], *o0[3:7])
        g1 = _C.render_tris_backward(*args, gc, gd, o1[0], *o1[3:7])
        for k, a, b in zip(TRI_NAMES, g0, g1):
            e = rel_err(b.cpu().numpy(), a.cpu().numpy())
            print(f"\ncall {call} dL_d{k}: rel_err {e:.2e}, bit-identical: {th.equal(a, b)}")
            assert e <= sum_order_tol(k), (call, k, e)


def test_band(oracle, hip_device):
    from dmesh_renderer_amd import _C
    L, n, B, H, W, _ = TRI_CASES["band"]
    rows = (1, 4)
    d = scenes.layered_sheets(L, n, B, H, W, seed=7, opacity=(0.1, 0.5))
    args = c_args(d, hip_device)
    for call in range(2):
        ff, bf, cf = _frag(_C.render_tris(*args, H, W, fragments=K))
        fb, bb, cb = _frag(_C.render_tris(*args, H, W, rows=rows, fragments=K))
        m = FR.band_rows(H, rows)
        assert (~m).any() and (fb[:, :, ~m] == -1).all() and (cb[:, ~m] == 0).all() and (bb[:, :, :, ~m] == 0).all()
        assert np.array_equal(fb[:, :, m], ff[:, :, m]) and np.array_equal(cb[:, m], cf[:, m])
        assert np.array_equal(bb[:, :, :, m].view(np.uint32), bf[:, :, :, m].view(np.uint32))
        assert cb[:, m].max() > 0


def test_opaque_faces_and_early_stop(oracle, hip_device):
    """The scene of test_alpha_gpu.py::test_tri_alpha_opaque_faces_and_early_stop: (a) holds, and no fragment follows the
    face a pixel stops at (opacity 1, or T < T_EPS)."""
    L, n, B, H, W = 14, 6, 1, 96, 144
    d = scenes.layered_sheets(L, n, B, H, W, seed=3, opacity=(0.45, 0.9))
    d["faces_opacity"][::11] = 1.0
    k = 16
    sc, ost, (face, bary, count) = _check_state(oracle, hip_device, d, B, H, W, (0, 0), "opaque+deep", k=k)
    T = ost.get("final_T").reshape(B, H, W)
    assert (T == 0).any() and ((T > 0) & (T < 1e-4)).any() and (T == 1).any()
    used = face >= 0
    o = np.where(used, sc.faces_opacity.astype(np.float64)[np.where(used, face, 0)], 0.0)
    t_before = np.concatenate([np.ones((B, 1, H, W)), np.cumprod(1 - o, axis=1)[:, :-1]], axis=1)  # T in front of slot k
    assert not (used & (t_before < 1e-4)).any(), "a fragment behind the stopping face"
    stopped = T < 1e-4
    last = np.take_along_axis(np.cumprod(1 - o, axis=1), np.maximum(count - 1, 0)[:, None].astype(np.int64), axis=1)[:, 0]
    assert (last[stopped] < 1e-4).all()


def test_forward_skipped_pair(oracle, hip_device):
    """(a) on case 21192 of tests/tools/fuzz_campaign.py (tests/test_fuzz_gpu.py::test_skipped_pair_inside_a_run_of_records builds
    it): a sliver face whose denom is exactly 0 at one of the pixels it covers.  The forward skips that pair, so it is no
    fragment: counted as one it would add a blend the oracle's colour does not have.  (On the CPU, a float32 restatement
    of the kernel's walk over the oracle's rays finds one such pair in this scene and a deepest pixel of 15 pairs.)"""
    from test_fuzz_gpu import _soup
    rng = np.random.RandomState(21192)
    B = int(rng.randint(1, 4)); H = int(rng.randint(17, 260)); W = int(rng.randint(17, 300)); rng.rand()
    P = int(rng.randint(8, 600)); F = int(rng.randint(30, 3000))
    assert (B, H, W, P, F) == (1, 130, 259, 410, 1755)
    d = _soup(21192, P, F, B, H, W)
    if rng.rand() < 0.3:
        d["verts"] = d["verts"] * float(rng.uniform(0.05, 4.0))
    _, _, (face, bary, count) = _check_state(oracle, hip_device, d, B, H, W, (0, 0), "fuzz 21192", k=16)
    # the scene does hold such a pair: the forward's tile_hits count every covered pair below n_contrib, skipped ones too
    # (what the backward's record buffer is sized from), the fragments only the blended ones
    from dmesh_renderer_amd import _C
    args = c_args(d, hip_device)
    out = _C.render_tris(*args, H, W)
    covered = int(_C.export("tile_hits", args, False, out[0], out[3:7], H, W, th.int32).sum())
    skipped = covered - int(count.sum())
    print(f"fuzz 21192: {covered} covered pairs below n_contrib, {int(count.sum())} fragments, {skipped} skipped by the forward")
    assert skipped >= 1, "the case no longer holds a covered pair with denom == 0"


def test_scanned_path(oracle, hip_device):
    """A frame above 8 192 tiles (test_alpha_gpu.py::test_tri_alpha_scanned_path's): lists sorted by k_sort_tiles.  The colour
    identity of (a), one call."""
    from dmesh_renderer_amd import _C
    L, n, B, H, W = 3, 40, 1, 1040, 2048
    assert ((H + 15) // 16) * ((W + 15) // 16) * B > 8192
    d = scenes.layered_sheets(L, n, B, H, W, seed=5, opacity=(0.1, 0.5))
    d["verts"] = d["verts"] * th.tensor([4.0, 4.0, 1.0])
    sc, ocolor, odepth, ost = _oracle(oracle, d, H, W)
    k = 4
    face, bary, count = _frag(_C.render_tris(*c_args(d, hip_device), H, W, fragments=k))
    assert int(count.max()) <= k
    color, _, _ = FR.composite64(sc, face, bary)
    e = float(np.abs(color - ocolor).max())
    print(f"\nscanned: fragments composite vs oracle colour {e:.2e}")
    assert e <= FWD_TOL and count.max() > 0


def test_async_and_graph(hip_device):
    from dmesh_renderer_amd import _C
    d, B, H, W = _deep_scene(W=144)
    args = c_args(d, hip_device)
    want = [t.clone() for t in _C.render_tris(*args, H, W, fragments=K)[7:10]]  # (also the warm-up: a default, waiting call)
    assert int(want[2].max()) > 2
    _C.set_async(True)
    try:
        got = _C.render_tris(*args, H, W, fragments=K)[7:10]
        th.cuda.synchronize()
    finally:
        _C.set_async(False)
    assert not _C.overflowed()
    for a, b in zip(got, want):
        assert th.equal(a, b)

    def step():
        out = _C.render_tris(*args, H, W, fragments=K)
        return (out[1],) + tuple(out[7:10])

    graph, captured, eager = capture_replay(step)
    for t in captured:
        t.zero_()
    replay(graph)
    for a, b in zip(captured[1:], want):
        assert th.equal(a, b)
    assert th.equal(captured[0], eager[0])


def test_module_and_helpers_through_autograd(oracle, hip_device):
    """composite(...) + T bg is the Module's colour; a loss on it gives the renderer's own gradients of verts_color,
    faces_opacity and faces_intense; face_visibility sums to B H W - sum(T)."""
    import dmesh_renderer_amd as dmr
    from dmesh_renderer_amd import fragments as FG
    dev = hip_device
    L, n, B, H, W, _ = TRI_CASES["two_views_ragged"]
    d = scenes.layered_sheets(L, n, B, H, W, seed=7, opacity=(0.1, 0.5))
    t = {k: v.to(dev) for k, v in d.items()}
    gc, gd = upstream_grads(B, H, W)
    gcd = gc.to(dev)
    names = ("verts_color", "faces_opacity", "faces_intense")
    r = dmr.TriRenderer(dmr.TriRenderSettings(H, W, t["bg"]), return_alpha=True, return_fragments=K)
    own = {k: t[k].clone().requires_grad_(True) for k in names}
    color, depth, alpha, frag = r(*(own.get(k, t[k]) for k in TRI_ARGS))
    th.autograd.backward([color], [gcd])
    color, alpha, g_own = color.detach(), alpha.detach(), {k: own[k].grad for k in names}
    assert isinstance(frag, dmr.Fragments) and tuple(alpha.shape) == (B, 1, H, W)
    assert not any(x.requires_grad for x in frag) and int(frag.count.max()) <= K
    lv = {k: t[k].clone().requires_grad_(True) for k in names}
    comp, T = FG.composite(frag, t["faces"], lv["faces_opacity"], lv["verts_color"], face_scale=lv["faces_intense"])
    mine = comp + T * t["bg"].view(1, 3, 1, 1)
    e = float((mine.detach() - color).abs().max())
    ea = float((1 - T.detach() - alpha).abs().max())
    print(f"\ncomposite + T bg vs the Module's colour {e:.2e}; 1 - T vs alpha {ea:.2e}")
    assert e <= FWD_TOL and ea <= FWD_TOL
    (mine * gcd).sum().backward()
    for k in names:
        eg = rel_err(lv[k].grad.cpu().numpy(), g_own[k].cpu().numpy())
        print(f"torch-side dL_d{k} vs the renderer's backward {eg:.2e}")
        assert eg <= GRAD_TOL, k
    vis = FG.face_visibility(frag, t["faces_opacity"], t["faces"].shape[0])
    assert tuple(vis.shape) == (B, t["faces"].shape[0])
    ev = abs(float(vis.detach().double().sum()) - (B * H * W - float(T.detach().double().sum())))
    print(f"face_visibility sum vs B H W - sum T: {ev:.2e} (bound {1e-5 * B * H * W:.2e})")
    assert ev <= 1e-5 * B * H * W
    # without alpha the Fragments are still the last output
    out = dmr.TriRenderer(dmr.TriRenderSettings(H, W, t["bg"]), return_fragments=2)(*(t[k] for k in TRI_ARGS))
    assert len(out) == 3 and isinstance(out[2], dmr.Fragments) and tuple(out[2].pix_to_face.shape) == (B, 2, H, W)


def test_bad_k(hip_device):
    from dmesh_renderer_amd import _C
    L, n, B, H, W, _ = TRI_CASES["one_view"]
    args = c_args(scenes.layered_sheets(L, n, B, H, W, seed=7), hip_device)
    for k in (33, -1):
        with pytest.raises(RuntimeError, match=r"0\.\.32"):
            _C.render_tris(*args, H, W, fragments=k)
