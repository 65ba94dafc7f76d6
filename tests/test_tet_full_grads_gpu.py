"""Full tet gradients on the GPU (DMR_FLAG_TET_FULL_GRADS / TetRenderer(full_grads=True)): dL/dverts and
dL/dfaces_intense of both backward kernels against the float64 brute-force reference of tests/tet_grad_ref.py, on the
pixels that reference keeps (the upstream gradients of every other pixel are zeroed on both sides).

Bounds: dL_dverts rel_err <= 1e-3, dL_dfintense <= 1e-4 (rel_err: max-abs error over max(1, max-abs reference)); the
full path's verts_color / faces_opacity within 1e-5 of the default path's; the re-marching and the sequence kernel
within 1e-5 of each other.  The errors measured on the MI355X are printed by each case (pytest -s) and recorded in
the docstring of test_full_grads_match_float64_reference.
"""
import pytest
import torch as th

from grad_cases import FINT_TOL, SAME_TOL, TET_CASES as CASES, TET_VERTS_TOL as VERTS_TOL, reference, scene, seq_state
from harness import capture_replay, module_step, replay, run_ablation_child, run_ranks
from util import c_args, rel_err, upstream_grads

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", list(CASES))
def test_full_grads_match_float64_reference(oracle, hip_device, case):
    """First call of a view configuration (no march sequence yet: the re-marching k_tet_backward) and second call
    (k_tet_backward_seq on the forward's sequence), each with full gradients and with the default ones.
    Measured on the MI355X (rel_err dL_dverts / dL_dfintense, call 0 and call 1; kept pixels):
      small             5.8e-6 / 2.0e-7, 4.6e-6 / 2.1e-7  (97 %)
      two_views_ragged  4.8e-6 / 3.7e-7, 4.9e-6 / 3.8e-7  (97 %)
      opaque            1.7e-6 / 5.3e-7, 1.7e-6 / 5.3e-7  (92 %)
      jitter            1.2e-5 / 1.9e-7, 9.7e-6 / 2.4e-7  (96 %)
    No criterion on grazing hits (small |den|) was needed.  tet_grad_ref already drops rays that pass within EDGE_EPS of
    a face edge, because the reference's reverse march stops early along them."""
    from dmesh_renderer_amd import _C
    d, B, H, W, seed = scene(case, W_extra=16 * (6 + list(CASES).index(case)))  # a view configuration of its own
    ref, gc, gd, rg = reference(oracle, d, B, H, W, seed)
    args = c_args(d, hip_device, tet=True)
    gcd, gdd = gc.to(hip_device), gd.to(hip_device)
    fulls = []
    for call in range(2):
        out = _C.render_tets(*args, H, W, seed)
        gf = _C.render_tets_backward(*args, gcd, gdd, *out[3:7], full_grads=True)
        g0 = _C.render_tets_backward(*args, gcd, gdd, *out[3:7])
        th.cuda.synchronize()
        longest, cap = seq_state(_C, args, out[3:7], H, W)
        assert (cap == 0) if call == 0 else (0 < longest <= cap), (call, longest, cap)
        gf = [x.cpu().numpy() for x in gf]
        assert gf[0].shape == (d["verts"].shape[0], 3) and gf[3].shape == (B, d["faces"].shape[0])
        ev, ei = rel_err(gf[0], rg["verts"]), rel_err(gf[3], rg["faces_intense"])
        print(f"\n{case} call {call}: dL_dverts {ev:.2e}  dL_dfintense {ei:.2e}  kept {ref.kept_fraction:.3f}")
        assert ev <= VERTS_TOL, (call, ev)
        assert ei <= FINT_TOL, (call, ei)
        for a, b_ in zip(gf[1:3], g0):
            assert rel_err(a, b_.cpu().numpy()) <= SAME_TOL
        fulls.append(gf)
    for a, b_ in zip(fulls[0], fulls[1]):  # re-march vs sequence kernel
        assert rel_err(a, b_) <= SAME_TOL


def test_module_full_grads_two_views(oracle, hip_device):
    """TetRenderer(full_grads=True) through autograd, B = 2."""
    import dmesh_renderer_amd as dmr
    d, B, H, W, seed = scene("two_views_ragged")
    ref, gc, gd, rg = reference(oracle, d, B, H, W, seed)
    t = {k: v.to(hip_device) for k, v in d.items()}
    r = dmr.TetRenderer(dmr.TetRenderSettings(H, W, t["bg"], seed), full_grads=True)
    _, g = module_step(r, t, ("verts", "verts_color", "faces_opacity", "verts_depth", "faces_intense"),
                       [gc.to(hip_device), gd.to(hip_device)])
    assert g["verts_depth"] is None
    assert rel_err(g["verts"].cpu().numpy(), rg["verts"]) <= VERTS_TOL
    assert rel_err(g["faces_intense"].cpu().numpy(), rg["faces_intense"]) <= FINT_TOL
    assert rel_err(g["verts_color"].cpu().numpy(), rg["verts_color"]) <= 1e-4


def test_full_grads_step_replays_as_graph(hip_device):
    """One forward + full-gradient backward captured with torch.cuda.graph matches the eager call."""
    from dmesh_renderer_amd import _C
    d, B, H, W, seed = scene("small", W_extra=16 * 12)
    args = c_args(d, hip_device, tet=True)
    gc, gd = upstream_grads(B, H, W)
    gcd, gdd = gc.to(hip_device), gd.to(hip_device)

    def step():
        out = _C.render_tets(*args, H, W, seed)
        return _C.render_tets_backward(*args, gcd, gdd, *out[3:7], full_grads=True)

    graph, captured, eager = capture_replay(step)
    replay(graph)
    for a, b_ in zip(captured, eager):
        assert rel_err(a.cpu().numpy(), b_.cpu().numpy()) <= SAME_TOL


def test_full_grads_direct_atomic_fallback(hip_device):
    """All 20 values per (pixel, face) through the direct atomics: the ablation build (harness.run_ablation_child) refuses odd
    faces a table slot (as tests/test_fallback_gpu.py does for the default gradients)."""
    run_ablation_child("tet_full", "full fallback ok")


def test_two_ranks_full_grads_match_single_rank(hip_device):
    """ShardedTetRenderer(full_grads=True) on two ranks (gloo, one GPU) against TetRenderer(full_grads=True) alone."""
    run_ranks("full_grads", "sharded full grads ok")
