"""fragments.surface_packed_fused on the GPU (csrc/dmr_surface.hip: k_surface_packed, k_surface_packed_backward) against
fragments.surface_packed evaluated in float64 on the CPU, on the same float32 inputs cast up; hit against interpolate_packed_fused
bit for bit; through the C ABI between sentinel words with verts one float off a 16-byte boundary; on rendered tri and tet lists,
alone and in the chain surface -> EnvMap -> blend; and through a replayed HIP graph.

Bound and metric (the row units'): an output is within max(its floor, 4 x the yardstick) of the float64 model, the floor 1e-5 for
hit / normal / reflect and 1e-4 for the gradients, the yardstick the float32 model on the CPU against the float64 one on the same
case, the metric row_units.rel_to_largest.  Nothing is derived from what the kernels give.  Rows with |m . d| < 1e-3, where
float32 and float64 may turn the normal to opposite sides, are left out of the comparison of `normal` and get no upstream of it
(surface_cases.lists; tests/test_surface_cpu.py holds their share below 2 % of every case); hit, reflect and every gradient are
compared on every row.  Every case prints what it measured beside its bound (pytest -s).

MEASURED on the MI355X, the largest figure over its 41 tests (rel_to_largest against the float64 model; every bound was its floor):
hit 1.2e-7, normal 1.5e-6, reflect 1.6e-6, dL_dverts 5.5e-6, dL_dbary 1.0e-6, dL_dorigin 5.6e-7 -- each beside a float32 torch
yardstick of the same size (1.5e-6, 1.5e-6, 5.4e-6 on the case of the largest three).  hit equals interpolate_packed_fused bit for
bit on all four cases; the call with verts one float off a 16-byte boundary gives the aligned call's three outputs bit for bit.
Graph replays against eager (used slots 6 306 -> 3 324 -> 8 242 of capacity 8 415): the stored outputs equal, dL_dverts to 3.8e-8,
dL_dorigin to 7.1e-8, exact zeros in the tail rows and in the vertex rows no slot touched.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch as th

import dmesh_renderer_amd as dmr
import surface_cases as SC
from dmesh_renderer_amd import Fragments, scenes
from dmesh_renderer_amd import fragments as FG
from harness import TET_ARGS, TRI_ARGS, capture_replay, replay
from row_units import FWD_TOL, GRAD_TOL, YARDSTICKS, check, guarded, intact
from row_units import rel_to_largest as _rel
from util import rel_err

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------
# The model, once per case: the three outputs and the gradients of each upstream alone (a sum of them is any subset's)
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _model(c):
    out, d = {}, SC.lists(c)
    for dtype in (th.float64, th.float32):
        lv = [d[k].to(dtype).clone().requires_grad_(True) for k in SC.GRADS]
        s = FG.surface_packed(Fragments(d["face"], lv[1], None), d["packed"], d["faces"], lv[0], lv[2])
        r = {k: x.detach().numpy() for k, x in zip(SC.OUTPUTS, s)}
        for x, u in zip(s, SC.UPSTREAMS):
            grads = th.autograd.grad((x * th.nan_to_num(d[u]).to(dtype)).sum(), lv, retain_graph=True, allow_unused=True)
            for k, leaf, gx in zip(SC.GRADS, lv, grads):
                r[k, u] = (th.zeros_like(leaf) if gx is None else gx).numpy()
        out[dtype] = r
    return out


def _without_near(c, x):
    x = np.array(x)
    x[SC.lists(c)["near"].numpy()] = 0
    return x


def _expect(c, ups=SC.UPSTREAMS, want=SC.GRADS):
    """(reference, bounds) of a call whose upstreams `ups` arrive and whose gradients `want` are asked for."""
    m = _model(c)
    pick = lambda r: dict({k: (_without_near(c, r[k]) if k == "normal" else r[k]) for k in SC.OUTPUTS}, **{k: sum(r[k, u] for u in ups) for k in want})
    ref, f32 = pick(m[th.float64]), pick(m[th.float32])
    bounds = {}
    for k in ref:
        yard = _rel(f32[k], ref[k])
        bounds[k] = (max(FWD_TOL if k in SC.OUTPUTS else GRAD_TOL, YARDSTICKS * yard), yard)
    return ref, bounds


def _pack_on(d, dev):
    p = FG.pack_slots_fused(Fragments(d["face"].to(dev), None, None), d["pack_f"], d["capacity"])
    assert p.rows == d["packed"].rows and th.equal(p.row.cpu(), d["packed"].row) and th.equal(p.n_used.cpu(), d["packed"].n_used)
    return p


def _fused(c, dev, ups=SC.UPSTREAMS, want=SC.GRADS):
    """surface_packed_fused on the device: the upstreams `ups` arrive (NaN in every row no counting slot holds), the gradients
    `want` are asked for -> {name: numpy}, `normal` with the rows near s = 0 zeroed as the reference's."""
    d = SC.lists(c)
    t = {k: d[k].to(dev) for k in ("face", "bary", "faces", "verts", "origin") + SC.UPSTREAMS}
    lv = {k: t[k].clone().requires_grad_(True) for k in want}
    s = FG.surface_packed_fused(Fragments(t["face"], lv.get("bary", t["bary"]), None), _pack_on(d, dev), t["faces"], lv.get("verts", t["verts"]),
                                lv.get("origin", t["origin"]))
    assert isinstance(s, FG.SurfaceRows) and all(tuple(x.shape) == (d["packed"].rows, 3) and x.dtype == th.float32 for x in s)
    got = {k: x.detach().cpu().numpy() for k, x in zip(SC.OUTPUTS, s)}
    got["normal"] = _without_near(c, got["normal"])
    if want and ups:
        outs = [x for x, u in zip(s, SC.UPSTREAMS) if u in ups]
        grads = th.autograd.grad(outs, [lv[k] for k in want], grad_outputs=[t[u] for u in ups])
        got.update({k: g.cpu().numpy() for k, g in zip(want, grads)})
    return got


def _run(what, c, dev, **kw):
    ref, bounds = _expect(c, **kw)
    got = _fused(c, dev, **kw)
    assert set(got) == set(ref)
    d = SC.lists(c)
    print(f"\n{what}: {d['count']} used slots, {d['packed'].rows} rows, {int(d['near'].sum())} of them left out of `normal`")
    check(what, ref, bounds, got, _rel)
    return ref, got


# ---------------------------------------------------------------------------
# (1) the table, capacities, another F, the special faces
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("c", SC.TABLE, ids=str)
def test_table(hip_device, c):
    ref, got = _run(f"{c.size} K {c.K} {c.frame}", c, hip_device)
    assert all(float(np.abs(ref[k]).max()) > 0 for k in ref)


@pytest.mark.parametrize("c", SC.CAPACITY, ids=lambda c: f"cap{c.cap:+d}")
def test_capacity(hip_device, c):
    """Capacity below, at and above the count, NaN in the tail rows of all three upstreams: the tail rows are exact zeros."""
    ref, got = _run(f"capacity {c.cap:+d}", c, hip_device)
    d = SC.lists(c)
    u = min(d["count"], d["packed"].rows)
    for k in SC.OUTPUTS:
        assert float(np.abs(got[k][u:]).sum()) == 0.0 and float(np.abs(got[k][:u]).max()) > 0
    assert (c.cap <= 0) == (u == d["packed"].rows) and all(bool(th.isnan(d[k][u:]).all()) for k in SC.UPSTREAMS)


def test_packed_for_a_larger_f(hip_device):
    """A `packed` made for F + 4 faces: the slots of faces F .. F + 3 have rows, do not count, and get three rows of zeros."""
    c = SC.OTHER_F
    ref, got = _run("packed for a larger F", c, hip_device)
    d = SC.lists(c)
    free = ~d["held"].numpy()
    assert 100 < int(free.sum()) < d["packed"].rows and all(float(np.abs(got[k][free]).sum()) == 0.0 for k in SC.OUTPUTS)


def test_degenerate_faces(hip_device):
    c = SC.DEGENERATE
    ref, got = _run("degenerate faces", c, hip_device)
    d = SC.lists(c)
    rows = d["packed"].row[th.isin(d["face"], th.tensor([1, 2], dtype=th.int32)) & (d["packed"].row >= 0)].long().numpy()
    w = got["hit"][rows] - d["origin"].numpy()[0]
    assert len(rows) > 100 and float(np.abs(got["normal"][rows]).max()) == 0.0
    assert float(np.abs(got["reflect"][rows] - w / np.linalg.norm(w, axis=1, keepdims=True)).max()) <= 1e-6


def test_face_with_a_vertex_out_of_range(hip_device):
    c = SC.BAD_VERTEX
    ref, got = _run("three faces with a vertex outside [0, P)", c, hip_device)
    d = SC.lists(c)
    P = d["verts"].shape[0]
    bad = ((d["faces"] < 0) | (d["faces"] >= P)).any(1)
    hit = (d["packed"].row >= 0) & (d["face"] >= 0) & (d["face"] < len(bad)) & bad[d["face"].clamp(0, len(bad) - 1).long()]
    rows = d["packed"].row[hit].long().numpy()
    assert int(bad.sum()) == 3 and len(rows) > 100 and all(float(np.abs(got[k][rows]).sum()) == 0.0 for k in SC.OUTPUTS)


def test_a_hit_at_the_camera_centre(hip_device):
    c = SC.AT_ORIGIN
    ref, got = _run("a hit at the camera centre", c, hip_device)
    r = int(SC.lists(c)["packed"].row[0, 0, 0, 0])
    assert float(np.abs(got["reflect"][r]).max()) == 0.0 and (got["hit"][r] == SC.lists(c)["origin"].numpy()[0]).all()


# ---------------------------------------------------------------------------
# (2) what is wanted, and what arrives
# ---------------------------------------------------------------------------
SUBSETS = [tuple(x for i, x in enumerate(range(3)) if m >> i & 1) for m in range(8)]


@pytest.mark.parametrize("m", range(8), ids=lambda m: "+".join(SC.GRADS[i] for i in SUBSETS[m]) or "none")
def test_every_subset_of_wanted_gradients(hip_device, monkeypatch, m):
    """Each subset reaches its own instantiation of the backward kernel; an output that is not wanted is not allocated."""
    from dmesh_renderer_amd import _C
    want = tuple(SC.GRADS[i] for i in SUBSETS[m])
    seen = []
    real = _C.surface_packed_backward
    monkeypatch.setattr(_C, "surface_packed_backward", lambda *a: seen.append(a[-1]) or real(*a))
    _run(f"wanted: {want or 'none'}", SC.SUBSETS, hip_device, want=want)
    assert seen == ([tuple(g in want for g in SC.GRADS)] if want else [])


@pytest.mark.parametrize("m", range(1, 8), ids=lambda m: "+".join(SC.OUTPUTS[i] for i in SUBSETS[m]))
def test_every_subset_of_arriving_upstreams(hip_device, monkeypatch, m):
    """An output the loss does not use sends nothing down: its upstream reaches the C call as a null pointer."""
    from dmesh_renderer_amd import _C
    ups = tuple(SC.UPSTREAMS[i] for i in SUBSETS[m])
    seen = []
    real = _C.surface_packed_backward
    monkeypatch.setattr(_C, "surface_packed_backward", lambda *a: seen.append(tuple(x is not None for x in a[7:10])) or real(*a))
    _run(f"upstreams: {ups}", SC.SUBSETS, hip_device, ups=ups)
    assert seen == [tuple(u in ups for u in SC.UPSTREAMS)]


# ---------------------------------------------------------------------------
# (3) hit is interpolate_packed_fused, bit for bit
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("c", [SC.TABLE[2], SC.TABLE[4], SC.CAPACITY[2], SC.BAD_VERTEX], ids=str)
def test_hit_is_the_packed_units_interpolation(hip_device, c):
    dev, d = hip_device, SC.lists(c)
    t = {k: d[k].to(dev) for k in ("face", "bary", "faces", "verts", "origin")}
    frag, packed = Fragments(t["face"], t["bary"], None), _pack_on(d, dev)
    hit = FG.surface_packed_fused(frag, packed, t["faces"], t["verts"], t["origin"]).hit
    rows = FG.interpolate_packed_fused(frag, packed, t["faces"], t["verts"])
    same = th.equal(hit, rows)
    print(f"\n{c}: hit vs interpolate_packed_fused(verts): equal {same}, largest difference {float((hit - rows).abs().max()):.2e} (max |hit| {float(rows.abs().max()):.3g})")
    assert float(rows.abs().max()) > 0 and same


# ---------------------------------------------------------------------------
# (4) the C ABI between sentinels, verts one float off a 16-byte boundary
# ---------------------------------------------------------------------------
def _c_pair(lib, dev, c, off):
    d = SC.lists(c)
    B, K, H, W = d["face"].shape
    F, P, N = d["faces"].shape[0], d["verts"].shape[0], d["packed"].rows
    stream = th.cuda.current_stream(dev).cuda_stream
    ints = {k: d[k].to(dev).contiguous() for k in ("face", "faces")}
    ints.update(row=d["packed"].row.to(dev).contiguous(), n_used=d["packed"].n_used.to(dev))
    sizes = dict(bary=d["bary"].numel(), verts=3 * P, origin=3 * B, hit=3 * N, normal=3 * N, reflect=3 * N, grad_hit=3 * N, grad_normal=3 * N,
                 grad_reflect=3 * N, dL_dverts=3 * P, dL_dbary=d["bary"].numel(), dL_dorigin=3 * B)
    bufs = {k: guarded(dev, n, off) for k, n in sizes.items()}
    for k in ("bary", "verts", "origin") + SC.UPSTREAMS:
        bufs[k][1].copy_(d[k].to(dev).flatten())
    p = {k: b[1].data_ptr() for k, b in bufs.items()}
    p.update({k: v.data_ptr() for k, v in ints.items()})
    head = (B, K, H, W, P, F, N, p["face"], p["bary"], p["row"], p["n_used"], p["faces"], p["verts"], p["origin"])
    with th.cuda.device(dev):
        assert lib.dmr_surface_packed(*head, p["hit"], p["normal"], p["reflect"], stream) == 0, lib.dmr_last_error()
        assert lib.dmr_surface_packed_backward(*head, p["grad_hit"], p["grad_normal"], p["grad_reflect"], p["dL_dverts"], p["dL_dbary"],
                                               p["dL_dorigin"], stream) == 0, lib.dmr_last_error()
    th.cuda.synchronize()
    for k, n in sizes.items():
        assert intact(bufs[k][0], n, off), k
    shape = dict(dL_dbary=tuple(d["bary"].shape), dL_dverts=(P, 3), dL_dorigin=(B, 3))
    names = dict(zip(SC.OUTPUTS, SC.OUTPUTS), dL_dverts="verts", dL_dbary="bary", dL_dorigin="origin")
    return {names[k]: bufs[k][1].cpu().numpy().reshape(shape.get(k, (N, 3))) for k in names}


def test_misaligned_verts_between_sentinels(hip_device):
    from dmesh_renderer_amd import _C
    c, dev = SC.MISALIGNED, hip_device
    lib = SC.declare(C.CDLL(_C.library_path()))
    ref, bounds = _expect(c)
    aligned, shifted = _c_pair(lib, dev, c, 0), _c_pair(lib, dev, c, 1)
    for k in SC.OUTPUTS:
        assert np.array_equal(aligned[k], shifted[k]), k
    for name, got in (("aligned", aligned), ("one float off", shifted)):
        check(f"C ABI, {name}", ref, bounds, dict(got, normal=_without_near(c, got["normal"])), _rel)


# ---------------------------------------------------------------------------
# (5) rendered lists
# ---------------------------------------------------------------------------
def _rendered(dev, r, t, args, name, K):
    """On a renderer's lists (return_fragments=K, fragment_grads=True): normal and reflect against the float64 model on the CPU
    (bound as above; rows within 1e-3 of s = 0 left out of `normal`), then the chain surface -> EnvMap -> blend against the same
    chain with the torch model in the middle, on the device: image, verts.grad, mv_mats.grad (through camera_origins), envmap.grad."""
    F = t["faces"].shape[0]
    th.manual_seed(4)
    env = FG.EnvMap(4, 8).to(dev)
    with th.no_grad():
        env.envmap.normal_()
    g_image, res = None, []
    for fused in (True, False):
        verts, mv_mats = t["verts"].clone().requires_grad_(True), t["mv_mats"].clone().requires_grad_(True)
        frag = r(*({"verts": verts, "mv_mats": mv_mats}.get(k, t[k]) for k in args))[-1]
        assert frag.bary.requires_grad and frag.pix_to_face.shape[1] == K
        packed = FG.pack_slots_fused(frag, F, frag.pix_to_face.numel())
        origin = FG.camera_origins(mv_mats)
        s = (FG.surface_packed_fused if fused else FG.surface_packed)(frag, packed, t["faces"], verts, origin)
        rgb = env(s.reflect, n_rows=packed.n_used)
        image, T = FG.composite_values_packed_fused(frag, packed, t["faces_opacity"], rgb)
        if g_image is None:
            g_image = th.randn(image.shape, generator=th.Generator().manual_seed(6)).to(dev)
            cpu = Fragments(frag.pix_to_face.cpu(), frag.bary.detach().cpu().double(), None)
            pk = FG.PackedSlots(packed.row.cpu(), packed.n_used.cpu(), packed.rows)
            m64 = FG.surface_packed(cpu, pk, t["faces"].cpu(), t["verts"].cpu().double(), origin.detach().cpu().double())
            m32 = FG.surface_packed(cpu._replace(bary=cpu.bary.float()), pk, t["faces"].cpu(), t["verts"].cpu(), origin.detach().cpu())
            d64 = m64.reflect - 2 * (m64.reflect * m64.normal).sum(1, keepdim=True) * m64.normal
            near = (((m64.normal * d64).sum(1).abs() < SC.NEAR) & (m64.normal.abs().sum(1) > 0)).numpy()
            n = int(packed.n_used)
            assert 500 < n <= packed.rows and near.sum() <= SC.NEAR_SHARE * n
            for k in SC.OUTPUTS:
                ref, f32, got = (np.array(getattr(x, k).detach().cpu().numpy()) for x in (m64, m32, s))
                if k == "normal":
                    ref[near], f32[near], got[near] = 0, 0, 0
                yard = _rel(f32, ref)
                e, bound = _rel(got, ref), max(FWD_TOL, YARDSTICKS * yard)
                print(f"\n{name} lists ({n} rows, {int(near.sum())} near s = 0): {k} {e:.2e} (float32 torch {yard:.2e}, bound {bound:.1e})")
                assert float(np.abs(ref).max()) > 0 and e <= bound, (k, e)
        grads = th.autograd.grad((image * g_image).sum(), [verts, mv_mats, env.envmap])
        res.append([image.detach().cpu().numpy()] + [g.cpu().numpy() for g in grads])
    for k, a, b in zip(("image", "verts", "mv_mats", "envmap"), *res):
        e = rel_err(a, b)
        print(f"\n{name} chain surface -> EnvMap -> blend: {k} {e:.2e} (max |ref| {float(np.abs(b).max()):.3g})")
        assert float(np.abs(b).max()) > 0 and float(np.abs(a).max()) > 0 and e <= (FWD_TOL if k == "image" else GRAD_TOL), (k, e)


def test_rendered_tri_lists(hip_device):
    dev, K, Hs, Ws = hip_device, 4, 40, 56
    t = {k: v.to(dev) for k, v in scenes.layered_sheets(3, 6, 2, Hs, Ws, seed=7, opacity=(0.1, 0.4)).items()}
    assert t["mv_mats"].shape[0] == 2
    r = dmr.TriRenderer(dmr.TriRenderSettings(Hs, Ws, t["bg"]), return_fragments=K, fragment_grads=True)
    _rendered(dev, r, t, TRI_ARGS, "tri", K)


def test_rendered_tet_lists(hip_device):
    dev, K, Hs, Ws = hip_device, 4, 48, 72
    t = {k: v.to(dev) for k, v in scenes.kuhn_tets(2, 1, Hs, Ws, seed=5).items()}
    r = dmr.TetRenderer(dmr.TetRenderSettings(Hs, Ws, t["bg"], 0), return_fragments=K, fragment_grads=True)
    _rendered(dev, r, t, TET_ARGS, "tet", K)


# ---------------------------------------------------------------------------
# (6) graph replay
# ---------------------------------------------------------------------------
def test_graph_replay(hip_device):
    """Forward + backward of pack (capacity=M) -> surface captured into one HIP graph and replayed twice over verts, origin and
    lists rewritten in place: the stored outputs (hit, normal, reflect, dL_dbary, row, n_used) equal the eager ones, the accumulated
    ones (dL_dverts, dL_dorigin) are within the gradient floor, and the vertex rows no slot touched are exact zeros."""
    dev, c = hip_device, SC.GRAPH
    d = SC.lists(c)
    F, P = d["faces"].shape[0], d["verts"].shape[0]
    M = d["face"].numel()
    t = {k: d[k].to(dev).clone() for k in ("face", "faces")}
    g = th.Generator().manual_seed(5)
    ups = {k: th.randn(M, 3, generator=g).to(dev) for k in SC.UPSTREAMS}
    lv = {k: d[k].to(dev).clone().requires_grad_(True) for k in SC.GRADS}
    names = SC.OUTPUTS + SC.GRADS + ("row", "n_used")

    def step():
        frag = Fragments(t["face"], lv["bary"], None)
        packed = FG.pack_slots_fused(frag, F, capacity=M)
        s = FG.surface_packed_fused(frag, packed, t["faces"], lv["verts"], lv["origin"])
        grads = th.autograd.grad(list(s), [lv[k] for k in SC.GRADS], grad_outputs=[ups[k] for k in SC.UPSTREAMS])
        return [x.detach() for x in s] + list(grads) + [packed.row, packed.n_used]

    def same(captured, eager, what):
        by, n = dict(zip(names, captured)), int(captured[-1])
        for k, a, b in zip(names, captured, eager):
            if k in ("verts", "origin"):
                e = _rel(a.cpu().numpy(), b.cpu().numpy())
                print(f"\ngraph replay vs eager, {what}, dL_d{k}: {e:.2e} (bound {GRAD_TOL:.0e}, max |eager| {float(b.abs().max()):.3g})")
                assert float(b.abs().max()) > 0 and e <= GRAD_TOL, (what, k, e)
            else:
                a, b = (a[:n], b[:n]) if k in SC.OUTPUTS else (a, b)
                eq = th.equal(a, b)
                print(f"\ngraph replay vs eager, {what}, {k}: equal {eq}")
                assert eq, (what, k)
        touched = th.zeros(P, dtype=th.bool, device=dev)
        live = (t["face"] >= 0) & (t["face"] < F)
        touched[t["faces"][t["face"][live].long()].long().flatten()] = True
        assert 0 < n < M and all(float(by[k][n:].abs().max()) == 0.0 and float(by[k][:n].abs().max()) > 0 for k in SC.OUTPUTS)
        assert 0 < int((~touched).sum()) and float(by["verts"][~touched].abs().max()) == 0.0 and float(by["verts"][touched].abs().max()) > 0
        return n

    graph, captured, eager = capture_replay(step)
    for x in captured:
        x.fill_(1)
    replay(graph)
    counts = [same(captured, eager, "the captured inputs")]
    for fraction in (0.6, 0.02):   # most of the slots emptied; then nearly all of them back
        with th.no_grad():
            r = th.rand(d["face"].shape, generator=g)
            t["face"].copy_(th.where(r < fraction, th.full_like(d["face"], -1), th.randint(0, F, d["face"].shape, generator=g, dtype=th.int32)).to(dev))
            lv["bary"].copy_((th.rand(d["bary"].shape, generator=g) * 0.45 + 0.02).to(dev))
            lv["verts"].copy_(th.rand(P, 3, generator=g).to(dev))
            lv["origin"].copy_((th.randn(d["origin"].shape, generator=g) + 3.0).to(dev))
        replay(graph)
        fresh = [x.detach().clone() for x in step()]
        th.cuda.synchronize()
        counts.append(same(captured, fresh, f"lists rewritten in place, {fraction:.0%} emptied"))
    print(f"used slots over the replays: {counts} of capacity {M}")
    assert counts[1] < counts[0] < counts[2] < M


def test_binding_refusals_name_this_call(hip_device):
    """The binding's own refusals, below fragments.py's (reached by direct callers of _C alone): each names surface_packed or the
    tensor of this call that is wrong, never the interpolate call whose argument block it shares.  No call reaches a kernel."""
    from dmesh_renderer_amd import _C
    dev, d = hip_device, SC.lists(SC.TABLE[0])
    t = {k: d[k].to(dev) for k in ("face", "bary", "faces", "verts", "origin")}
    good = dict(t, row=d["packed"].row.to(dev), n_used=d["packed"].n_used.to(dev), rows=d["packed"].rows)
    order = ("face", "bary", "row", "n_used", "faces", "verts", "origin", "rows")
    B, _, H, W = t["face"].shape
    for change, text in ((dict(verts=t["verts"][:, :2]), "verts must have dimensions (num_points, 3)"), (dict(verts=t["verts"].cpu()), "verts must be on the device of pix_to_face"),
                         (dict(verts=t["verts"].double()), "(verts)"), (dict(origin=t["origin"][0]), "origin must have dimensions (B, 3)"),
                         (dict(origin=t["origin"].cpu()), "origin must be on the device of pix_to_face"), (dict(rows=-1), "surface_packed: rows must be in 0..2^31 - 1, got -1"),
                         (dict(face=t["face"].expand(B, 33, H, W), bary=t["bary"].expand(B, 33, 2, H, W), row=good["row"].expand(B, 33, H, W)),
                          "surface_packed: K must be in 1..32, got 33")):
        with pytest.raises(RuntimeError) as e:
            _C.surface_packed(*(dict(good, **change)[k] for k in order))
        assert text in str(e.value) and "interpolate" not in str(e.value) and "vert_attrs" not in str(e.value), (text, str(e.value))
