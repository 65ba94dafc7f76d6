"""The tet renderer's per-pixel fragment lists on the GPU (DMR_FLAG_TET_FRAGMENTS; `fragments=K` of render_tets;
return_fragments=K of TetRenderer; helpers in dmesh_renderer_amd/fragments.py) against the CPU oracle's forward state and
against the float64 model of tests/tet_grad_ref.py (checks: tests/tet_fragments_ref.py).

Bounds: forward quantities 1e-5 absolute (FWD_TOL, the project's); face ids, counts and everything the option must not move:
exact; two backward paths over the same sums SAME_TOL (1e-5), torch-side against renderer gradients rel_err <= 1e-4.  The
barycentrics against the float64 model: four times the float32 noise of the formula itself, measured in the test (see
test_oracle_state_and_model), never less than FWD_TOL.  Every case prints what it measured (pytest -s).
"""
import numpy as np
import pytest
import torch as th

import tet_fragments_ref as TF
from dmesh_renderer_amd import scenes
from fragments_ref import band_rows
from grad_cases import SAME_TOL, TET_CASES, scene, seq_state
from harness import TET_ARGS, capture_replay, replay
from tet_grad_ref import TetGradRef
from util import c_args, rel_err, upstream_grads

pytestmark = pytest.mark.gpu

FWD_TOL = TF.FWD_TOL
GRAD_TOL = 1e-4
K = 32
EXPORTS = (("n_contrib", th.int32), ("first_face", th.int32), ("last_face", th.int32), ("is_active", th.uint8), ("final_T", th.int32),
           ("final_prev_T", th.int32))

_cases = {}


def _case(oracle, case):
    """The scene of a TET_CASES entry, the oracle's forward of it and (unjittered cases) the float64 model: computed once."""
    if case not in _cases:
        d, B, H, W, seed = scene(case)
        sc = oracle.scene_from_module_inputs(d, H, W, seed=seed)
        ocolor, odepth, oactive, ost = oracle.tet_forward(sc)
        ref = None
        if seed == 0:
            ref = TetGradRef(d, H, W, ost)
            assert ref.kept_fraction >= 0.8, ref.kept_fraction
        _cases[case] = (d, B, H, W, seed, sc, ocolor, odepth, ost, ref)
    return _cases[case]


def _frag(out):
    """face, bary, count of a render_tets(fragments=K) tuple as numpy."""
    assert len(out) == 10
    face, bary, count = (t.cpu().numpy() for t in out[7:10])
    assert face.dtype == np.int32 and bary.dtype == np.float32 and count.dtype == np.int32
    return face, bary, count


def _estimate(longest):
    """The capacity the next forward of the view configuration takes from a longest march (dmr_api.hip: + 25 % + 4, up to 4)."""
    return (longest + longest // 4 + 4 + 3) // 4 * 4


def _check_model(ref, d, ost, face, bary, count, tag):
    """On the pixels the float64 model keeps: the stored faces are its faces_of[:, :steps], exactly, and bary is its float64
    (u, v) within four times what the same Moeller-Trumbore in numpy float32 on the oracle's rays deviates from it."""
    B, H, W = ref.B, ref.H, ref.W
    mface, mbary, mcount = TF.model_lists(ref, d["verts"], d["faces"])
    Kr = mface.shape[1]
    assert Kr <= face.shape[1]
    keep = ref.keep.reshape(B, H, W).numpy()
    kf = np.broadcast_to(keep[:, None], face.shape)
    assert np.array_equal(count[keep], mcount[keep])
    assert np.array_equal(face[:, :Kr][kf[:, :Kr]], mface[kf[:, :Kr]]) and (face[:, Kr:][kf[:, Kr:]] == -1).all()
    kb = np.broadcast_to(keep[:, None, None], mbary.shape)
    err = float(np.abs(bary[:, :Kr].astype(np.float64) - mbary)[kb].max())
    # the float32 noise of the formula: ray_tri_hit in numpy float32 on the oracle's float32 rays, over the same pairs
    pix = ref.pix.numpy()
    ro, rd = ost.get("ray_o").reshape(-1, 3)[pix], ost.get("ray_d").reshape(-1, 3)[pix]
    verts, faces = d["verts"].numpy(), d["faces"].numpy()
    m64 = mbary.transpose(0, 3, 4, 1, 2).reshape(-1, Kr, 2)[pix]  # [N, Kr, 2]
    noise = 0.0
    for k in range(Kr):
        live = (k < ref.steps).numpy()
        f = ref.faces_of[:, k].clamp(min=0).numpy()
        u, v = TF.hits32(ro, rd, verts[faces[f, 0]], verts[faces[f, 1]], verts[faces[f, 2]])
        dev = np.maximum(np.abs(u.astype(np.float64) - m64[:, k, 0]), np.abs(v.astype(np.float64) - m64[:, k, 1]))[live]
        noise = max(noise, float(dev.max()) if dev.size else 0.0)
    bound = max(4 * noise, FWD_TOL)
    print(f"\n{tag}: {int(keep.sum())} kept pixels ({ref.kept_fraction:.3f}), faces exact; bary vs float64 {err:.2e}; float32 noise of the "
          f"formula {noise:.2e}, bound {bound:.2e}")
    assert err <= bound, (err, noise)


@pytest.mark.parametrize("case", list(TET_CASES))
def test_oracle_state_and_model(oracle, hip_device, case):
    """K = 32 on two calls of the view configuration (a backward between them leaves the estimate the second is sized from; the
    first has its capacity raised to 32 if the configuration is new): shapes, the oracle's state, the float64 composite, pixels
    that marched and then failed, and the float64 model.  Measured on the CPU oracle: longest march 21 / 28 / 8 / 28, pixels that
    marched and failed 399 / 254 / 68 / 0, kept fractions 0.975 / 0.964 / 0.924 (small / two_views_ragged / opaque / jitter).
    Measured on the MI355X (both calls alike): composite against the oracle, colour 1.7e-7 / 2.3e-7 / 1.5e-7 / 2.3e-7, depth
    4.2e-7 / 3.3e-7 / 1.8e-7 / 3.4e-7, final T 7.6e-8 / 7.1e-8 / 1.0e-8 / 7.1e-8; bary against the float64 model 1.55e-5 / 1.45e-5 /
    1.03e-5, equal to the float32 noise of the formula measured here (bounds 6.2e-5 / 5.8e-5 / 4.1e-5)."""
    from dmesh_renderer_amd import _C
    d, B, H, W, seed, sc, ocolor, odepth, ost, ref = _case(oracle, case)
    args = c_args(d, hip_device, tet=True)
    gc, gd = upstream_grads(B, H, W)
    nc = ost.get("n_contrib").astype(np.int64).reshape(B, H, W)
    act = ost.get("is_active").reshape(B, H, W) != 0
    failed = ~act & (nc > 0)
    print(f"\n{case}: longest march {int(nc.max())} (active pixels {int(nc[act].max())}), {int(failed.sum())} pixels marched and then failed")
    for call in range(2):
        out = _C.render_tets(*args, H, W, seed, fragments=K)
        face, bary, count = _frag(out)
        assert face.shape == (B, K, H, W) and bary.shape == (B, K, 2, H, W) and count.shape == (B, H, W)
        assert int(count.max()) <= K
        TF.check_state(ost, face, bary, count)
        TF.check_composite(sc, ost, ocolor, odepth, face, bary, count, tag=f"{case} call {call}")
        longest, cap = seq_state(_C, args, out[3:7], H, W)
        assert longest == int(nc.max()) and cap >= K and cap % 4 == 0, (longest, cap)
        if call == 1:
            assert cap == max(K, _estimate(longest)), (longest, cap)
        if seed == 0:
            assert failed.any() and (count[failed] == 0).all() and (face[:, 0][failed] == -1).all()
            _check_model(ref, d, ost, face, bary, count, f"{case} call {call}")
        _C.render_tets_backward(*args, gc.to(hip_device), gd.to(hip_device), *out[3:7])
        th.cuda.synchronize()


def test_truncation(oracle, hip_device):
    """fragments=4 and fragments=6 (no multiple of 4) against fragments=32 on "small": the same counts, the first K slots bit
    for bit."""
    from dmesh_renderer_amd import _C
    d, B, H, W, seed = _case(oracle, "small")[:5]
    args = c_args(d, hip_device, tet=True)
    for call in range(2):
        f32, b32, c32 = _frag(_C.render_tets(*args, H, W, seed, fragments=32))
        deep = float((c32 > 8).mean())
        print(f"\ncall {call}: {100 * deep:.0f} % of the pixels deeper than 8")
        assert deep > 0.25
        for k in (4, 6):
            fk, bk, ck = _frag(_C.render_tets(*args, H, W, seed, fragments=k))
            assert fk.shape == (B, k, H, W) and np.array_equal(ck, c32)
            assert np.array_equal(fk, f32[:, :k]) and np.array_equal(bk.view(np.uint32), b32[:, :k].view(np.uint32))


@pytest.mark.parametrize("k,w_extra", [(8, 64), (32, 80)])
def test_capacity_and_the_backward(oracle, hip_device, k, w_extra):
    """The first call of a view configuration of its own: the march sequence has room for exactly K rounded up to 4 steps.
    fragments=8: cap == 8 < longest, the lists are still the oracle's, and the backward of that forward re-marches on the
    device's decision; fragments=32: cap == 32 >= longest, the backward takes the sequence on call 0.  Either equals the
    backward of a forward without the flag to SAME_TOL."""
    from dmesh_renderer_amd import _C
    d, B, H, W, seed = scene("small", W_extra=w_extra)
    sc = oracle.scene_from_module_inputs(d, H, W, seed=seed)
    _, _, _, ost = oracle.tet_forward(sc)
    args = c_args(d, hip_device, tet=True)
    gc, gd = (t.to(hip_device) for t in upstream_grads(B, H, W))
    out = _C.render_tets(*args, H, W, seed, fragments=k)
    g = _C.render_tets_backward(*args, gc, gd, *out[3:7])
    th.cuda.synchronize()
    longest, cap = seq_state(_C, args, out[3:7], H, W)
    print(f"\nfragments={k}, first call: longest march {longest}, capacity {cap}")
    assert longest == int(ost.get("n_contrib").max())
    assert (cap == 8 < longest) if k == 8 else (cap == 32 >= longest), (longest, cap)
    face, bary, count = _frag(out)
    TF.check_state(ost, face, bary, count)
    assert (count > k).any() if k == 8 else int(count.max()) <= k
    out0 = _C.render_tets(*args, H, W, seed)
    g0 = _C.render_tets_backward(*args, gc, gd, *out0[3:7])
    th.cuda.synchronize()
    assert len(out0) == 7 and 0 < longest <= seq_state(_C, args, out0[3:7], H, W)[1]  # (sized from the estimate: the sequence path)
    for name, a, b in zip(("verts_color", "faces_opacity"), g, g0):
        e = rel_err(a.cpu().numpy(), b.cpu().numpy())
        print(f"dL_d{name}: flagged forward's backward vs plain forward's {e:.2e}")
        assert e <= SAME_TOL, (name, e)


def test_nothing_else_moves(oracle, hip_device):
    """A warm view configuration, with and without alpha: images bit for bit, the exports the backward reads equal, the
    gradients within SAME_TOL (the tet tests' bound for two paths over the same sums)."""
    from dmesh_renderer_amd import _C
    d, B, H, W, seed = _case(oracle, "small")[:5]
    args = c_args(d, hip_device, tet=True)
    gc, gd = (t.to(hip_device) for t in upstream_grads(B, H, W))
    for _ in range(2):
        out = _C.render_tets(*args, H, W, seed)
        _C.render_tets_backward(*args, gc, gd, *out[3:7])
    for akw in ({}, {"alpha": True}):
        o0 = _C.render_tets(*args, H, W, seed, **akw)
        o1 = _C.render_tets(*args, H, W, seed, fragments=8, **akw)
        assert len(o0) == 7 and len(o1) == 10
        for a, b in zip(o0[:3], o1[:3]):
            assert a.shape == b.shape and th.equal(a, b), "colour / depth (/ alpha) / active must not change with the option"
        assert tuple(o1[1].shape) == (B, 2 if akw else 1, H, W)
        for name, dt in EXPORTS:
            x0, x1 = (_C.export(name, args, True, 0, o[3:7], H, W, dt) for o in (o0, o1))
            assert th.equal(x0, x1), name
        assert seq_state(_C, args, o0[3:7], H, W) == seq_state(_C, args, o1[3:7], H, W)
        gdd = th.cat([gd, 0.5 * gd], 1) if akw else gd
        g0 = _C.render_tets_backward(*args, gc, gdd, *o0[3:7], **akw)
        g1 = _C.render_tets_backward(*args, gc, gdd, *o1[3:7], **akw)
        for name, a, b in zip(("verts_color", "faces_opacity"), g0, g1):
            e = rel_err(b.cpu().numpy(), a.cpu().numpy())
            print(f"\nalpha {bool(akw)} dL_d{name}: rel_err {e:.2e}, bit-identical: {th.equal(a, b)}")
            assert e <= SAME_TOL, (name, e)


def test_band(oracle, hip_device):
    from dmesh_renderer_amd import _C
    d, B, H, W, seed = _case(oracle, "two_views_ragged")[:5]
    rows = (2, 6)
    args = c_args(d, hip_device, tet=True)
    for call in range(2):
        ff, bf, cf = _frag(_C.render_tets(*args, H, W, seed, fragments=K))
        fb, bb, cb = _frag(_C.render_tets(*args, H, W, seed, rows=rows, fragments=K))
        m = band_rows(H, rows)
        assert (~m).any() and (fb[:, :, ~m] == -1).all() and (cb[:, ~m] == 0).all() and (bb[:, :, :, ~m] == 0).all()
        assert np.array_equal(fb[:, :, m], ff[:, :, m]) and np.array_equal(cb[:, m], cf[:, m])
        assert np.array_equal(bb[:, :, :, m].view(np.uint32), bf[:, :, :, m].view(np.uint32))
        assert cb[:, m].max() > 0
    print(f"\nband rows {rows}: {int((cb[:, m] > 0).sum())} pixels with fragments inside, none outside")


def test_async_and_graph(oracle, hip_device):
    from dmesh_renderer_amd import _C
    d, B, H, W, seed = _case(oracle, "small")[:5]
    args = c_args(d, hip_device, tet=True)
    want = [t.clone() for t in _C.render_tets(*args, H, W, seed, fragments=K)[7:10]]  # (also the warm-up: a default, waiting call)
    assert int(want[2].max()) > 8
    _C.set_async(True)
    try:
        got = _C.render_tets(*args, H, W, seed, fragments=K)[7:10]
        th.cuda.synchronize()
    finally:
        _C.set_async(False)
    assert not _C.overflowed()
    for a, b in zip(got, want):
        assert th.equal(a, b)

    def step():
        out = _C.render_tets(*args, H, W, seed, fragments=K)
        return (out[0],) + tuple(out[7:10])

    graph, captured, eager = capture_replay(step)
    for t in captured:
        t.zero_()
    replay(graph)
    for a, b in zip(captured[1:], want):
        assert th.equal(a, b)
    assert th.equal(captured[0], eager[0])
    print(f"\nasync and graph replay reproduce the lists ({int(want[2].sum())} counted faces)")


def test_module_and_helpers_through_autograd(oracle, hip_device):
    """composite(...) + T bg is the Module's colour, on inactive pixels too, and 1 - T its alpha; a loss on it gives the
    renderer's own gradients of verts_color, faces_opacity and faces_intense; face_visibility sums to B H W - sum(T).
    The upstream gradient is masked to the pixels the float64 model keeps, as in every tet gradient test here
    (grad_cases.reference): along the other rays the renderer's reverse march may stop early, as the reference's does
    (tests/tet_grad_ref.py), and the faces in front of the stop get no gradient from it."""
    import dmesh_renderer_amd as dmr
    from dmesh_renderer_amd import fragments as FG
    dev = hip_device
    d, B, H, W, seed, sc, ocolor, odepth, ost, ref = _case(oracle, "two_views_ragged")
    t = {k: v.to(dev) for k, v in d.items()}
    gcd = (upstream_grads(B, H, W)[0] * ref.mask()).to(dev)
    names = ("verts_color", "faces_opacity", "faces_intense")
    r = dmr.TetRenderer(dmr.TetRenderSettings(H, W, t["bg"], seed), full_grads=True, return_alpha=True, return_fragments=K)
    own = {k: t[k].clone().requires_grad_(True) for k in names}
    color, depth, active, alpha, frag = r(*(own.get(k, t[k]) for k in TET_ARGS))
    th.autograd.backward([color], [gcd])
    color, alpha, g_own = color.detach(), alpha.detach(), {k: own[k].grad for k in names}
    assert isinstance(frag, dmr.Fragments) and tuple(alpha.shape) == (B, 1, H, W) and active.dtype == th.bool
    assert not any(x.requires_grad for x in frag) and int(frag.count.max()) <= K
    assert (~active).any() and (frag.count[~active] == 0).all() and (frag.count[active] > 0).all()
    lv = {k: t[k].clone().requires_grad_(True) for k in names}
    comp, T = FG.composite(frag, t["faces"], lv["faces_opacity"], lv["verts_color"], face_scale=lv["faces_intense"])
    mine = comp + T * t["bg"].view(1, 3, 1, 1)
    e = float((mine.detach() - color).abs().max())
    ei = float((mine.detach() - color).abs().permute(0, 2, 3, 1)[~active].max())
    ea = float((1 - T.detach() - alpha).abs().max())
    print(f"\ncomposite + T bg vs the Module's colour {e:.2e} (inactive pixels {ei:.2e}); 1 - T vs alpha {ea:.2e}")
    assert e <= FWD_TOL and ea <= FWD_TOL
    (mine * gcd).sum().backward()
    for k in names:
        eg = rel_err(lv[k].grad.cpu().numpy(), g_own[k].cpu().numpy())
        print(f"torch-side dL_d{k} vs the renderer's backward {eg:.2e}")
        assert eg <= GRAD_TOL, k
    F = t["faces"].shape[0]
    vis = FG.face_visibility(frag, t["faces_opacity"], F)
    assert tuple(vis.shape) == (B, F)
    ev = abs(float(vis.detach().double().sum()) - (B * H * W - float(T.detach().double().sum())))
    print(f"face_visibility sum vs B H W - sum T: {ev:.2e} (bound {1e-5 * B * H * W:.2e})")
    assert ev <= 1e-5 * B * H * W
    # without alpha the Fragments are still the last output
    out = dmr.TetRenderer(dmr.TetRenderSettings(H, W, t["bg"], seed), return_fragments=2)(*(t[k] for k in TET_ARGS))
    assert len(out) == 4 and isinstance(out[3], dmr.Fragments) and tuple(out[3].pix_to_face.shape) == (B, 2, H, W)


def test_bad_k_and_empty_inputs(hip_device):
    from dmesh_renderer_amd import _C
    m, B, H, W = 4, 1, 64, 80
    d = scenes.kuhn_tets(m, B, H, W, seed=0)
    args = c_args(d, hip_device, tet=True)
    for k in (33, -1):
        with pytest.raises(RuntimeError, match=r"0\.\.32"):
            _C.render_tets(*args, H, W, 0, fragments=k)
    dd = dict(d)
    dd["verts"] = d["verts"][:0]; dd["verts_color"] = d["verts_color"][:0]; dd["verts_depth"] = d["verts_depth"][:, :0]
    dd["faces"] = d["faces"][:0]; dd["faces_opacity"] = d["faces_opacity"][:0]; dd["faces_intense"] = d["faces_intense"][:, :0]
    dd["face_tets"] = d["face_tets"][:0]; dd["tets"] = d["tets"][:0]; dd["tet_faces"] = d["tet_faces"][:0]
    out = _C.render_tets(*c_args(dd, hip_device, tet=True), H, W, 0, fragments=4)
    th.cuda.synchronize()
    face, bary, count = _frag(out)
    assert face.shape == (B, 4, H, W) and (face == -1).all() and (bary == 0).all() and (count == 0).all()
    assert float(out[2].abs().max()) == 0.0
    print("\nP == 0: -1 / 0 throughout")


def test_malformed_tets(oracle, hip_device):
    """The scene of test_tet_parity_gpu.py::test_malformed_tets_stop_the_march_like_the_reference: the oracle-state checks
    hold, and the marches that stop inside the mesh have no fragments."""
    from dmesh_renderer_amd import _C
    m, B, H, W = 5, 1, 112, 128
    d = scenes.kuhn_tets(m, B, H, W, seed=3, opacity=(0.05, 0.4))
    tf = d["tet_faces"].clone()
    T = tf.shape[0]
    tf[3::11, 1] = tf[3::11, 0]           # the same face in two slots of a tet
    tf[5::13, 2] = tf[(7 + 5) % T, 0]     # a face of some other tet in the third slot
    d["tet_faces"] = tf.contiguous()
    sc = oracle.scene_from_module_inputs(d, H, W)
    _, _, oactive, ost = oracle.tet_forward(sc)
    args = c_args(d, hip_device, tet=True)
    stopped = (oactive.reshape(B, H, W) == 0) & (ost.get("n_contrib").reshape(B, H, W) > 0)
    assert stopped.any(), "the scene must have marches that stop inside the mesh"
    for call in range(2):
        face, bary, count = _frag(_C.render_tets(*args, H, W, 0, fragments=K))
        assert int(count.max()) <= K
        TF.check_state(ost, face, bary, count)
        assert (count[stopped] == 0).all()
    print(f"\nmalformed tets: {int(stopped.sum())} pixels stopped inside the mesh, all without fragments; longest list {int(count.max())}")
