"""fragments.envmap_rows_fused, EnvMap and pixel_directions on the GPU (csrc/dmr_envmap.hip: k_envmap_rows, k_envmap_rows_backward;
csrc/dmr_rows_common.hip: k_rows_fill) against fragments.envmap_rows evaluated in float64 on the CPU, on the same float32 inputs
cast up: the case table of tests/envmap_cases.py (every instantiation; N around a wave, a workgroup's tile and the capped grid;
C = 1 .. 16; maps from 1 x 1 to 64 x 128; directions uniform, in a 2-degree cone, all the same, at the seam, at the caps,
shuffled), special rows between sentinels, d, y and the map off a 16-byte boundary, n_rows on the device, single gradients, the
sum identity, a replayed HIP graph, the pixel directions of rendered lists, and the two chains of the module docstring.

Inputs: |d| in [0.5, 3], map and upstream ~ N(0,1).  Errors are max |got - ref| / max |ref| (_rel, which is row_units.rel_to_largest).
Bounds (the project's own): y within max(FWD_TOL = 1e-5, 4 x the yardstick), gradients within max(GRAD_TOL = 1e-4, 4 x the
yardstick), the yardstick being fragments.envmap_rows in float32 on the CPU against float64 on the same case; never anything the
kernels gave.  For the dL_dd comparison only, rows within 1e-3 texel of a cell line or with rho2 < 1e-4 carry no upstream
(envmap_cases.no_dd_upstream; at most 2 % of a case's rows, asserted): there float32 and float64 may sit in different cells and
the derivative, which holds the cell constant, jumps.  Every case prints what it measured (pytest -s).

MEASURED on the MI355X, the largest figure over the table's 28 cases (in brackets float32 torch on the CPU on the same cases, the
yardstick): y 1.0e-5 (1.2e-5), dL_dd 5.2e-6 (6.6e-6), dL_denvmap 6.1e-6 (1.1e-5); at most 1.17 % of a case's rows without upstream in
the dL_dd comparison.  The 4 misaligned calls give the aligned calls' y and dL_dd bit for bit, dL_denvmap too.  Special rows: y 7.5e-7,
dL_dd 1.9e-7, dL_denvmap 8.2e-7, exact zeros in the skipped rows, every sentinel word unchanged.  n_rows: at most 2.3e-6.  A single
gradient alone: dL_dd equal to the pair's, dL_denvmap within 3.7e-8.  Graph replays against eager (n_rows 500 -> 90 -> 700 of 700
rows): y and dL_dd equal, dL_denvmap within 6.1e-8 and 1.9e-6 from float64, exact zeros in the 55, 324 and 260 texels no row touched.
Pixel directions on 3 685 interior slots of two views: 3.0e-7 from the hit points' directions (float32 yardstick 2.3e-7).  The
background chain (4 480 rows): image 6.9e-7, envmap.grad 4.9e-7, faces_opacity.grad 1.2e-7, mv_mats.grad 2.0e-7.  The packed-row
chain (15 795 rows of 59 904 with capacity=M): image 2.9e-7, verts.grad 1.5e-6, envmap.grad 5.8e-7.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch as th

import envmap_cases as EC
import dmesh_renderer_amd as dmr
from dmesh_renderer_amd import fragments as FG
from dmesh_renderer_amd import scenes
from harness import TRI_ARGS, capture_replay, replay
from row_units import FWD_TOL, GRAD_TOL, check, counts_calls, declare, guarded, intact, models, n_rows_counts, within_floors
from row_units import rel_to_largest as _rel
from tri_grad_ref import pixel_rays
from util import rel_err, sum_order_tol

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _inputs(c, seed=0):
    """float32 CPU tensors of a case: d, envmap, the upstream, and the upstream of the dL_dd comparison."""
    d, env = EC.directions_of(c, seed), EC.envmap_of(c, seed)
    g = th.Generator().manual_seed(1000 * seed + 7 * c.N + 13 * c.C + c.He)
    up = th.randn(c.N, c.C, generator=g)
    quiet = th.from_numpy(EC.no_dd_upstream(d, c.He, c.We))
    return dict(d=th.from_numpy(d), env=th.from_numpy(env), up=up, up_d=th.where(quiet.unsqueeze(1), th.zeros(()), up), quiet=quiet)


def _run(f, c, t, device, dtype, n=None, want=None):
    """{"y", "d" (dL/dd, from the upstream without the rows near a cell line), "e" (dL/denvmap, from the full upstream)} of one
    forward and one backward per gradient, as numpy; n: the n_rows count or None; want: c.want unless given."""
    want = want or c.want
    d = t["d"].clone().to(device, dtype).requires_grad_("d" in want)       # (clones: on the CPU in float32 .to() is the cached tensor itself)
    env = t["env"].clone().to(device, dtype).requires_grad_("e" in want)
    nr = None if n is None else th.tensor([n], dtype=th.int32, device=device)
    y = f(d, env, n_rows=nr)
    out = {"y": y.detach().cpu().numpy()}
    if "d" in want:
        out["d"] = th.autograd.grad(y, [d], grad_outputs=t["up_d"].to(device, dtype), retain_graph="e" in want)[0].cpu().numpy()
    if "e" in want:
        out["e"] = th.autograd.grad(y, [env], grad_outputs=t["up"].to(device, dtype))[0].cpu().numpy()
    return out


@functools.lru_cache(maxsize=None)
def _models(c, n=None):
    """fragments.envmap_rows on the CPU in float64 and in float32 -> (reference, {name: (the bound of the case, the yardstick)})."""
    return models(_run, FG.envmap_rows, c._replace(want="de"), _inputs(c), n, _rel)


def _check(what, c, got, n=None):
    return check(what, *_models(c, n), got, _rel)


@pytest.mark.parametrize("i", range(len(EC.TABLE)))
def test_table(hip_device, i):
    c = EC.TABLE[i]
    t = _inputs(c)
    share = float(t["quiet"].float().mean()) if c.N else 0.0
    print(f"\n{c}: {100 * share:.2f} % of the rows carry no upstream in the dL_dd comparison")
    assert share <= 0.02
    got = _run(FG.envmap_rows_fused, c, t, hip_device, th.float32)
    ref = _check(str(c), c, got)
    if c.N == 0:
        assert ref["y"].shape == (0, c.C) and float(np.abs(got["e"]).max()) == 0.0
        return
    assert float(np.abs(ref["y"]).max()) > 0 and float(np.abs(ref["e"]).max()) > 0
    flat = c.We == 1 and (c.He == 1 or (c.layout == "caps" and c.He < 7))   # one column, and one row or the clamped rows of the caps: a constant
    assert flat or float(np.abs(ref["d"]).max()) > 0
    # the sum identity: the four weights of a row sum to 1.  Float32 sums of the upstream's terms: within 1e-5 (some 170
    # float32 roundings) of the sum of their magnitudes
    total, want = got["e"].astype(np.float64).sum((0, 1)), t["up"].double().sum(0).numpy()
    assert np.abs(total - want).max() <= 1e-5 * max(1.0, float(t["up"].abs().sum(0).max())), (total, want)


# ---------------------------------------------------------------------------
# Through the C ABI: sentinels, and buffers one float off a 16-byte boundary
# ---------------------------------------------------------------------------
def _c_calls():
    from dmesh_renderer_amd import _C
    return declare(C.CDLL(_C.library_path()), ["dmr_envmap_rows", "dmr_envmap_rows_backward"])


def _call_pair(lib, dev, N, Cn, He, We, d, env, up, off=0, n_rows=None):
    """One forward and one backward through the C ABI with every tensor inside a guarded buffer `off` floats off alignment
    -> (y [N,C], dL_dd [N,3], dL_denvmap [He,We,C]) as numpy; asserts that every sentinel is unchanged."""
    stream = th.cuda.current_stream(dev).cuda_stream
    sizes = dict(d=N * 3, env=He * We * Cn, y=N * Cn, up=N * Cn, dd=N * 3, de=He * We * Cn)
    bufs = {k: guarded(dev, n, off) for k, n in sizes.items()}
    bufs["d"][1].copy_(d.to(dev).flatten())
    bufs["env"][1].copy_(env.to(dev).flatten())
    bufs["up"][1].copy_(up.to(dev).flatten())
    p = {k: b[1].data_ptr() for k, b in bufs.items()}
    nr = None if n_rows is None else n_rows.data_ptr()
    with th.cuda.device(dev):
        assert lib.dmr_envmap_rows(N, Cn, He, We, p["d"], p["env"], nr, p["y"], stream) == 0, lib.dmr_last_error()
        assert lib.dmr_envmap_rows_backward(N, Cn, He, We, p["d"], p["env"], nr, p["up"], p["dd"], p["de"], stream) == 0, lib.dmr_last_error()
    th.cuda.synchronize()
    for k, n in sizes.items():
        assert intact(bufs[k][0], n, off), k
    return (bufs["y"][1].cpu().numpy().reshape(N, Cn), bufs["dd"][1].cpu().numpy().reshape(N, 3), bufs["de"][1].cpu().numpy().reshape(He, We, Cn))


@pytest.mark.parametrize("i", range(len(EC.MISALIGNED)))
def test_one_float_off_a_16_byte_boundary(hip_device, i):
    """The same call with every buffer at base + 4 bytes (no float4 reads): y and dL_dd bit-equal to the aligned call's,
    dL_denvmap within the suite's summation-order tolerance; the words around every buffer unchanged."""
    c, dev = EC.MISALIGNED[i], hip_device
    t, lib = _inputs(c), _c_calls()
    (y0, dd0, de0), (y1, dd1, de1) = (_call_pair(lib, dev, c.N, c.C, c.He, c.We, t["d"], t["env"], t["up_d"], off) for off in (0, 1))
    e_e = _rel(de1, de0)
    print(f"\n{c}: y equal {np.array_equal(y0, y1)}, dL_dd equal {np.array_equal(dd0, dd1)}, dL_denvmap {e_e:.2e} from the aligned call")
    assert np.array_equal(y0, y1) and np.array_equal(dd0, dd1) and e_e <= sum_order_tol("envmap")
    ref, bounds = _models(c)
    assert _rel(y1, ref["y"]) <= bounds["y"][0] and _rel(dd1, ref["d"]) <= bounds["d"][0]


def test_special_rows(hip_device):
    """Zero, NaN, +-Inf, 1e30, a denormal, the exact poles and the exact seam among ordinary rows, in every wave of three, with
    the map, y and both gradients inside larger buffers: finite results, exact zeros in y and dL_dd where the row is skipped, an
    exact-zero dL_dd at the poles, the model's values everywhere else, and every sentinel word unchanged.  The float64 reference
    holds a zero row where float32's |d|^2 leaves the format."""
    dev, nan, inf = hip_device, float("nan"), float("inf")
    Cn, He, We = EC.SPECIAL
    g = th.Generator().manual_seed(21)
    N = 192
    d = th.from_numpy(EC.directions_of(EC.case(N, Cn, He, We, "sphere"), seed=3)).clone()
    skipped, poles = th.zeros(N, dtype=th.bool), th.zeros(N, dtype=th.bool)
    rows = ([0, 0, 0], [nan, 0.3, 0.2], [inf, 0.0, 1.0], [0.1, -inf, nan], [1e30, 0.0, 0.0], [-1e30, 1e30, 1e30], [nan, nan, nan], [1e-40, 0.0, -1e-41],
            [0.0, 0.0, 1.0], [0.0, 0.0, -2.5], [-0.0, 0.0, 0.7], [-1.0, 0.0, 0.3], [-2.0, -0.0, 0.6])
    for k, row in enumerate(rows):
        for wave in range(3):
            r = 64 * wave + 4 * k + wave
            d[r] = th.tensor(row)
            skipped[r], poles[r] = k < 8, 8 <= k < 11
    env, up = th.randn(He, We, Cn, generator=g), th.randn(N, Cn, generator=g)
    up_d = th.where(th.from_numpy(EC.no_dd_upstream(th.where(skipped.unsqueeze(1), th.ones(()), d).numpy(), He, We)).unsqueeze(1), th.zeros(()), up)
    assert float((up_d != up).any(1).float().mean()) <= 0.08   # (the nine pole rows among them)
    y, dd, _ = _call_pair(_c_calls(), dev, N, Cn, He, We, d, env, up_d)
    _, _, de = _call_pair(_c_calls(), dev, N, Cn, He, We, d, env, up)
    d64 = th.where(skipped.unsqueeze(1), th.zeros(()), d).double().requires_grad_(True)
    e64 = env.double().requires_grad_(True)
    y64 = FG.envmap_rows(d64, e64)
    dd64, = th.autograd.grad(y64, [d64], grad_outputs=up_d.double(), retain_graph=True)
    de64, = th.autograd.grad(y64, [e64], grad_outputs=up.double())
    for k, a, b, tol in (("y", y, y64, FWD_TOL), ("dL_dd", dd, dd64, GRAD_TOL), ("dL_denvmap", de, de64, GRAD_TOL)):
        e = _rel(a, b.detach().numpy())
        print(f"\nspecial rows {k}: {e:.2e} (max |ref| {float(b.detach().abs().max()):.3g})")
        assert np.isfinite(a).all() and e <= tol, (k, e)
    s, p = skipped.numpy(), poles.numpy()
    assert float(np.abs(y[s]).max()) == 0.0 and float(np.abs(dd[s]).max()) == 0.0 and float(np.abs(dd[p]).max()) == 0.0
    assert float(np.abs(y[p]).max(1).min()) > 0 and float(np.abs(dd[~s & ~p]).max()) > 0
    assert np.array_equal(y[4 * 11], y[4 * 12])   # phi = +pi and phi = -pi: the same two columns, the same weights


# ---------------------------------------------------------------------------
# n_rows
# ---------------------------------------------------------------------------
def test_n_rows_on_the_device(hip_device):
    """The counts 0, below N, N, above N and negative, NaN in the tail rows of d and of the upstream: exact zeros in the tails of
    y and dL_dd, dL_denvmap the model's (nothing from the tail)."""
    c = EC.N_ROWS
    base = _inputs(c)
    for n in n_rows_counts(c.N):
        m = min(max(n, 0), c.N)
        t = dict(base, d=base["d"].clone(), up=base["up"].clone(), up_d=base["up_d"].clone())
        t["d"][m:], t["up"][m:], t["up_d"][m:] = float("nan"), float("nan"), float("nan")
        got = _run(FG.envmap_rows_fused, c, t, hip_device, th.float32, n)
        clean = {k: (th.nan_to_num(v) if v.dtype.is_floating_point else v) for k, v in t.items()}
        ref = _run(FG.envmap_rows, c, clean, "cpu", th.float64, n)
        within_floors(f"n_rows {n} of {c.N},", ref, got, _rel)
        assert float(np.abs(got["y"][m:]).sum()) == 0.0 and float(np.abs(got["d"][m:]).sum()) == 0.0
        if m == 0:
            assert all(float(np.abs(got[k]).max()) == 0.0 for k in got)
        else:
            assert all(float(np.abs(got[k][:m] if k != "e" else got[k]).max()) > 0 for k in got)


# ---------------------------------------------------------------------------
# Gradient subsets
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(EC.ONLY)))
def test_only_what_is_asked(hip_device, i):
    """Each gradient asked alone equals the pair's (dL_dd bit for bit, dL_denvmap within sum_order_tol) and the model's."""
    c = EC.ONLY[i]
    t = dict(_inputs(c))
    t["up"] = t["up_d"]   # one upstream for both gradients: the pair is then one backward call
    d = t["d"].to(hip_device).requires_grad_(True)
    env = t["env"].to(hip_device).requires_grad_(True)
    pair = th.autograd.grad(FG.envmap_rows_fused(d, env), [d, env], grad_outputs=t["up"].to(hip_device))
    only_d = _run(FG.envmap_rows_fused, c, t, hip_device, th.float32, want="d")
    only_e = _run(FG.envmap_rows_fused, c, t, hip_device, th.float32, want="e")
    e_e = _rel(only_e["e"], pair[1].cpu().numpy())
    print(f"\n{c}: only dL_dd equal {np.array_equal(only_d['d'], pair[0].cpu().numpy())}; only dL_denvmap {e_e:.2e} from the pair's")
    assert set(only_d) == {"y", "d"} and set(only_e) == {"y", "e"}
    assert np.array_equal(only_d["d"], pair[0].cpu().numpy()) and np.array_equal(only_d["y"], only_e["y"]) and e_e <= sum_order_tol("envmap")
    ref = _run(FG.envmap_rows, c, t, "cpu", th.float64)
    _, bounds = _models(c)
    assert _rel(only_d["d"], ref["d"]) <= bounds["d"][0] and _rel(only_e["e"], ref["e"]) <= bounds["e"][0]
    assert not FG.envmap_rows_fused(d.detach(), env.detach()).requires_grad


def test_no_upstream_launches_nothing(hip_device, monkeypatch):
    """An output the loss does not use reaches the Function's backward as None: Nones go down and the binding is not called."""
    from dmesh_renderer_amd import _C
    t = _inputs(EC.ONLY[0])
    d, env = t["d"].to(hip_device).requires_grad_(True), t["env"].to(hip_device).requires_grad_(True)
    y = FG.envmap_rows_fused(d, env)
    z = y * 1.0
    calls = counts_calls(monkeypatch, _C, "envmap_rows_backward")
    grads = th.autograd.grad((d * 3).sum(), [d, env], allow_unused=True)
    assert grads[1] is None and not calls
    assert FG._EnvMapRowsFn.backward(y.grad_fn, None) == (None, None, None) and not calls
    th.autograd.grad(z.sum(), [env])
    assert calls == [1]


# ---------------------------------------------------------------------------
# Graph replay
# ---------------------------------------------------------------------------
def test_graph_replay(hip_device):
    """Forward + backward captured into one HIP graph and replayed over d, envmap and n_rows rewritten in place, the count going
    down and up: y and dL_dd equal the eager ones exactly, dL_denvmap is within the gradient bound of the float64 model and holds
    an exact zero in every texel no row touched (the rows of the rewrites lie in one half of the sphere)."""
    dev, c = hip_device, EC.GRAPH
    t = _inputs(c)
    d = t["d"].to(dev).requires_grad_(True)
    env = t["env"].to(dev).requires_grad_(True)
    up, n_rows = t["up_d"].to(dev), th.tensor([500], dtype=th.int32, device=dev)
    names = ["y", "d", "e"]

    def step():
        y = FG.envmap_rows_fused(d, env, n_rows=n_rows)
        return [y.detach()] + list(th.autograd.grad(y, [d, env], grad_outputs=up))

    def same(captured, eager, what):
        n = min(max(int(n_rows), 0), c.N)
        d64, e64 = d.detach().double().cpu().requires_grad_(True), env.detach().double().cpu().requires_grad_(True)
        y64 = FG.envmap_rows(d64, e64, n_rows=n_rows.cpu())
        ref_e = th.autograd.grad(y64, [e64], grad_outputs=up.double().cpu())[0].numpy()
        k = EC.coords64(d.detach().cpu().numpy()[:n], c.He, c.We)
        touched = np.zeros((c.He, c.We), dtype=bool)
        for iy in ("iy0", "iy1"):
            for ix in ("ix0", "ix1"):
                touched[k[iy], k[ix]] = True
        near = min(np.minimum(k[f], 1 - k[f]).min() for f in ("fx", "fy")) if n else 1.0
        for name, a, b in zip(names, captured, eager):
            if name in ("y", "d"):
                print(f"\ngraph replay vs eager, {what}, {name}: equal {th.equal(a, b)}")
                assert th.equal(a, b), (what, name)
                assert float(a[n:].abs().sum()) == 0.0 and (n == 0 or float(a[:n].abs().max()) > 0)
            else:
                e, e_ref = _rel(a.cpu().numpy(), b.cpu().numpy()), _rel(a.cpu().numpy(), ref_e)
                print(f"\ngraph replay vs eager, {what}, {name}: {e:.2e} from eager, {e_ref:.2e} from float64; {int((~touched).sum())} texels untouched")
                assert e <= GRAD_TOL and e_ref <= GRAD_TOL, (what, name, e, e_ref)
                if near > 1e-4:   # (no row so close to a cell line that float32 could touch a neighbour)
                    assert float(np.abs(a.cpu().numpy()[~touched]).sum()) == 0.0

    graph, captured, eager = capture_replay(step)
    for x in captured:
        x.fill_(1)
    replay(graph)
    same(captured, eager, "the captured inputs")
    g = th.Generator().manual_seed(9)
    for n, half in ((90, 1.0), (c.N, -1.0)):
        with th.no_grad():
            w = th.randn(c.N, 3, generator=g)
            w[:, 2] = half * (w[:, 2].abs() + 0.3)           # one half of the sphere: the other half of the map is not touched
            w = w / w.norm(dim=1, keepdim=True) * (0.5 + 2.5 * th.rand(c.N, 1, generator=g))
            d.copy_(w.to(dev))
            env.copy_(th.randn(c.He, c.We, c.C, generator=g).to(dev))
            n_rows.fill_(n)
        replay(graph)
        fresh = [x.detach().clone() for x in step()]
        th.cuda.synchronize()
        same(captured, fresh, f"d, envmap and n_rows = {n} rewritten in place")


# ---------------------------------------------------------------------------
# Rendered lists: a slot's direction is its pixel's direction
# ---------------------------------------------------------------------------
def test_directions_of_rendered_tri_lists_are_the_pixel_directions(hip_device):
    """Two views with different cameras, fragment lists with barycentrics.  On slots strictly inside their face the hit point lies
    on the pixel's ray, so normalize(hit - camera_origins(mv)[view]) is pixel_directions at the slot's pixel.  The bound is the one
    of tests/test_sh_gpu.py's ray test: 4 x the float32 yardstick -- the larger of what the hit points' directions and float32
    pixel_directions on the CPU give against the float64 rays of tests/tri_grad_ref.py --, which itself stays below 1e-4."""
    dev, K, Hs, Ws = hip_device, 4, 40, 56
    t = {k: v.to(dev) for k, v in scenes.layered_sheets(3, 6, 2, Hs, Ws, seed=7, opacity=(0.1, 0.4)).items()}
    r = dmr.TriRenderer(dmr.TriRenderSettings(Hs, Ws, t["bg"]), return_fragments=K, fragment_grads=True)
    frag = r(*(t[k] for k in TRI_ARGS))[-1]
    packed = FG.pack_slots_fused(frag, t["faces"].shape[0])
    origin = FG.camera_origins(t["mv_mats"])
    view = FG.packed_row_views_fused(frag, packed)
    hit = FG.interpolate_packed_fused(frag, packed, t["faces"], t["verts"])
    w = (hit - origin[view.clamp(min=0).long()]).detach()
    got = (w / w.norm(dim=1, keepdim=True)).double().cpu()
    u, v = frag.bary[:, :, 0].detach().cpu(), frag.bary[:, :, 1].detach().cpu()
    row = packed.row.cpu()
    interior = (row >= 0) & (u > 1e-3) & (v > 1e-3) & (u + v < 1 - 1e-3)
    b, k, py, px = interior.nonzero(as_tuple=True)
    rows = row[interior].long()
    _, ray = pixel_rays(t["mv_mats"].double().cpu(), t["proj_mats"].double().cpu(), b, px, py, Hs, Ws)
    ray = ray / ray.norm(dim=1, keepdim=True)
    dirs = FG.pixel_directions(t["mv_mats"], t["proj_mats"], Hs, Ws)
    assert tuple(dirs.shape) == (2, Hs, Ws, 3) and dirs.is_cuda
    mine = dirs.double().cpu()[b, py, px]
    on_cpu = FG.pixel_directions(t["mv_mats"].cpu(), t["proj_mats"].cpu(), Hs, Ws).double()[b, py, px]
    yard = max(float((got[rows] - ray).abs().max()), float((on_cpu - ray).abs().max()))
    e_dirs, e = float((mine - ray).abs().max()), float((mine - got[rows]).abs().max())
    print(f"\npixel directions on {len(rows)} interior slots of two views: float32 yardstick {yard:.2e}; pixel_directions {e_dirs:.2e} from the "
          f"float64 rays, {e:.2e} from the hit points' directions")
    assert len(rows) > 500 and int((b == 0).sum()) > 100 and int((b == 1).sum()) > 100
    assert yard < 1e-4 and e_dirs <= 4 * yard and e <= 4 * yard
    assert float((dirs.double().cpu().flip(0)[b, py, px] - ray).abs().max()) > 0.1   # the other view's camera: the check above would fail


# ---------------------------------------------------------------------------
# The chains of the module docstring
# ---------------------------------------------------------------------------
def test_background_chain(hip_device):
    """image + T * env(pixel_directions) on rendered tri lists of two views, as the module docstring writes it, against the same
    chain with fragments.envmap_rows in the middle, on the device: the image, envmap.grad, faces_opacity.grad and mv_mats.grad."""
    dev, K, Hs, Ws = hip_device, 4, 40, 56
    t = {k: v.to(dev) for k, v in scenes.layered_sheets(3, 6, 2, Hs, Ws, seed=7, opacity=(0.1, 0.4)).items()}
    r = dmr.TriRenderer(dmr.TriRenderSettings(Hs, Ws, t["bg"]), return_fragments=K)
    B = t["mv_mats"].shape[0]
    th.manual_seed(4)
    env = FG.EnvMap(4, 8).to(dev)
    with th.no_grad():
        env.envmap.normal_()
    g_image, res = None, []
    for fused in (True, False):
        faces_opacity = t["faces_opacity"].clone().requires_grad_(True)
        mv_mats = t["mv_mats"].clone().requires_grad_(True)
        frag = r(*(faces_opacity if k == "faces_opacity" else t[k] for k in TRI_ARGS))[-1]
        image, T = FG.composite_fused(frag, t["faces"], faces_opacity, t["verts_color"])
        dirs = FG.pixel_directions(mv_mats, t["proj_mats"], Hs, Ws)
        if fused:
            bg = env(dirs.reshape(-1, 3)).view(B, Hs, Ws, 3).permute(0, 3, 1, 2)
        else:
            bg = FG.envmap_rows(dirs.reshape(-1, 3), env.envmap).view(B, Hs, Ws, 3).permute(0, 3, 1, 2)
        color = image + T * bg
        if g_image is None:
            g_image = th.randn(color.shape, generator=th.Generator().manual_seed(6)).to(dev)
        grads = th.autograd.grad((color * g_image).sum(), [env.envmap, faces_opacity, mv_mats])
        res.append([color.detach().cpu().numpy()] + [g.cpu().numpy() for g in grads])
    assert float(T.min()) > 0.05   # the background shines through everywhere
    for k, a, b in zip(("image", "envmap", "faces_opacity", "mv_mats"), *res):
        e = rel_err(a, b)
        print(f"\nbackground chain ({B * Hs * Ws} rows): {k} {e:.2e} (max |ref| {float(np.abs(b).max()):.3g})")
        assert float(np.abs(b).max()) > 0 and float(np.abs(a).max()) > 0 and e <= (FWD_TOL if k == "image" else GRAD_TOL), (k, e)


def test_packed_row_chain(hip_device):
    """A specular term over packed rows with fragment_grads=True: d = hit - origin[view], composite_values_packed_fused(...,
    env(d, n_rows=n)) with capacity=M, against the same chain with fragments.envmap_rows in the middle: the image and verts.grad
    (through dL_dd, the hit points and the renderer's backward)."""
    dev, K, Hs, Ws = hip_device, 4, 72, 104
    t = {k: v.to(dev) for k, v in scenes.layered_sheets(4, 8, 2, Hs, Ws, seed=3, opacity=(0.1, 0.4)).items()}
    r = dmr.TriRenderer(dmr.TriRenderSettings(Hs, Ws, t["bg"]), return_fragments=K, fragment_grads=True)
    F = t["faces"].shape[0]
    th.manual_seed(4)
    env = FG.EnvMap(4, 8).to(dev)
    with th.no_grad():
        env.envmap.normal_()
    g_image, res = None, []
    for fused in (True, False):
        verts = t["verts"].clone().requires_grad_(True)
        frag = r(*(verts if k == "verts" else t[k] for k in TRI_ARGS))[-1]
        packed = FG.pack_slots_fused(frag, F, frag.pix_to_face.numel())
        n = packed.n_used
        view = FG.packed_row_views_fused(frag, packed)
        hit = FG.interpolate_packed_fused(frag, packed, t["faces"], verts)
        d = hit - FG.camera_origins(t["mv_mats"])[view.clamp(min=0).long()]
        rgb = env(d, n_rows=n) if fused else FG.envmap_rows(d, env.envmap, n_rows=n)
        image, T = FG.composite_values_packed_fused(frag, packed, t["faces_opacity"], rgb)
        if g_image is None:
            g_image = th.randn(image.shape, generator=th.Generator().manual_seed(6)).to(dev)
        grads = th.autograd.grad((image * g_image).sum(), [verts, env.envmap])
        res.append([image.detach().cpu().numpy()] + [g.cpu().numpy() for g in grads])
        used = int(n)
    for k, a, b in zip(("image", "verts", "envmap"), *res):
        e = rel_err(a, b)
        print(f"\npacked-row chain ({used} rows of {packed.rows}): {k} {e:.2e} (max |ref| {float(np.abs(b).max()):.3g})")
        assert float(np.abs(b).max()) > 0 and float(np.abs(a).max()) > 0 and e <= (FWD_TOL if k == "image" else GRAD_TOL), (k, e)
