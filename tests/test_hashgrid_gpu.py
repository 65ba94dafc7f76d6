"""fragments.hashgrid_rows_fused and HashGrid on the GPU (csrc/dmr_hashgrid.hip: k_hashgrid_rows, k_hashgrid_rows_backward,
and csrc/dmr_rows_common.hip's k_rows_fill) against fragments.hashgrid_rows evaluated in float64 on the CPU, on the same float32 inputs cast up: the case
table of tests/hashgrid_cases.py (every instantiation; N around a wave, a workgroup's tile and the capped grid; dense, hashed and
mixed levels up to R = 4096; rows along a ramp, uniform, and all identical), y off a 16-byte boundary, special coordinates,
n_rows on the device, single gradients, the chain pack -> hit points -> HashGrid -> RowMLP -> blend on rendered lists, and a
replayed HIP graph.

Inputs: table ~ N(0,1), upstream ~ N(0,1), x as hashgrid_cases.rows_of.  dL/dx jumps at cell boundaries, so a row that has, at some
level, a coordinate within 8 * 2^-24 * R_l of one (hashgrid_cases.boundary_band: where floor(p) may differ between float32 and
float64) carries no upstream FOR THE dL/dx COMPARISON ONLY -- at most 3 % of a case's rows: asserted.  y and dL/dtable are
continuous there and are compared on every row, with the full upstream.

Bounds (the project's own): forward rel_err <= FWD_TOL = 1e-5, gradients rel_err <= GRAD_TOL = 1e-4 (scenes.rel_err).  Each
case also evaluates hashgrid_rows in float32 on the CPU and prints its distance from float64 -- the yardstick: t = p - i carries
6e-5 of float32 rounding at R = 2048 --, and a case's bound is the larger of the project's bound and four times that distance;
never anything the kernels gave.  Two evaluations of the same sums in another order: <= sum_order_tol(name).  Every case prints
what it measured (pytest -s).

MEASURED on the MI355X, the largest figure over the table's 26 cases (rel_err against the float64 model; in brackets float32
torch on the CPU on the same cases, the yardstick): y 2.1e-5 (2.1e-5), dL_dx 2.7e-5 (2.7e-5), dL_dtable 1.1e-5 (1.1e-5) -- the
figures ARE the yardstick's: both carry the float32 rounding of p = u R; on grids of power-of-two resolutions all three are at
or below 3e-7.  At most 12 of 1000 rows lie in the boundary band.  The 3 misaligned calls give the aligned calls' y and dL_dx
bit for bit, dL_dtable to 2.7e-8.  Special coordinates: y 4.7e-8, dL_dx 5.7e-8, dL_dtable 7.4e-8, exact zeros on clamped and NaN
coordinates.  n_rows: dL_dtable equals the truncated call's exactly.  A single gradient alone: dL_dx equal, dL_dtable to 3.6e-8.
The chains on rendered lists against the torch models in the middle (tri 9 674 rows of 35 840 with capacity=M; tet 5 472 of
13 824): image 6.0e-8, verts.grad 2.8e-7, table.grad 8.2e-8, the MLP's gradients to 2.7e-6.  Graph replays against eager (n_rows
500 -> 90 -> 700 of 700 rows): y and dL_dx equal, dL_dtable to 5.2e-8, exact zeros in the tail rows and in every table row no
point touched.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch as th

import hashgrid_cases as HC
from dmesh_renderer_amd import fragments as FG
from dmesh_renderer_amd import scenes
from harness import TET_ARGS, TRI_ARGS, capture_replay, replay
from row_units import FWD_TOL, GRAD_TOL, check, counts_calls, declare, guarded, intact, models, n_rows_counts, within_floors
from util import rel_err, sum_order_tol

pytestmark = pytest.mark.gpu

BAND_CAP = 0.03


def _spec(c):
    return FG.hashgrid_spec(c.L, c.F, c.log2_T, c.R0, c.s)


@functools.lru_cache(maxsize=None)
def _inputs(c, seed=0):
    """float32 CPU tensors of a case: x, table, the upstream, and the upstream with zeros in the rows of the boundary band."""
    spec = _spec(c)
    g = th.Generator().manual_seed(1000 * seed + 7 * c.N + 13 * c.L + c.F + c.log2_T)
    x = th.from_numpy(HC.rows_of(c, seed))
    table = th.randn(spec.offsets[-1], c.F, generator=g)
    up = th.randn(c.N, c.L * c.F, generator=g)
    band = th.from_numpy(HC.boundary_band(x.numpy(), spec.resolutions))
    assert int(band.sum()) <= BAND_CAP * max(c.N, 1) or c.N < 50, (c, int(band.sum()))
    up_x = up.clone()
    up_x[band] = 0
    return dict(x=x, table=table, up=up, up_x=up_x, band=int(band.sum()))


def _run(f, c, d, device, dtype, n=None, want="xt"):
    """{"y", "t" (dL/dtable under the full upstream), "x" and "tx" (dL/dx and dL/dtable of ONE call, under the upstream without
    the band's rows)} as numpy; n: the n_rows count or None.  want = "xt": the pair's instantiation (and the table-only one for
    "t"); "x" / "t": that gradient alone."""
    spec = _spec(c)
    x = d["x"].clone().to(device, dtype).requires_grad_("x" in want)          # (clones: on the CPU in float32 .to() is the cached tensor itself)
    table = d["table"].clone().to(device, dtype).requires_grad_("t" in want)
    nr = None if n is None else th.tensor([n], dtype=th.int32, device=device)
    y = f(x, table, spec, nr)
    out = {"y": y.detach().cpu().numpy()}
    if want == "xt":
        gx, gtx = th.autograd.grad(y, [x, table], grad_outputs=d["up_x"].to(device, dtype), retain_graph=True)
        out["x"], out["tx"] = gx.cpu().numpy(), gtx.cpu().numpy()
    elif want == "x":
        out["x"] = th.autograd.grad(y, [x], grad_outputs=d["up_x"].to(device, dtype))[0].cpu().numpy()
    if "t" in want:
        out["t"] = th.autograd.grad(y, [table], grad_outputs=d["up"].to(device, dtype))[0].cpu().numpy()
    return out


@functools.lru_cache(maxsize=None)
def _models(c, n=None):
    """fragments.hashgrid_rows on the CPU in float64 and in float32 -> (reference, {name: (the bound of the case, the yardstick)})."""
    return models(_run, FG.hashgrid_rows, c, _inputs(c), n, rel_err)


def _check(what, c, got, n=None):
    return check(what, *_models(c, n), got, rel_err)


@pytest.mark.parametrize("i", range(len(HC.TABLE)))
def test_table(hip_device, i):
    c = HC.TABLE[i]
    d = _inputs(c)
    print(f"\n{c}: {d['band']} of {c.N} rows in the boundary band")
    ref = _check(str(c), c, _run(FG.hashgrid_rows_fused, c, d, hip_device, th.float32))
    if c.N:
        assert all(float(np.abs(v).max()) > 0 for v in ref.values())
    else:
        assert ref["y"].shape == (0, c.L * c.F) and float(np.abs(ref["t"]).max()) == 0


# ---------------------------------------------------------------------------
# y (and the upstream) one float off a 16-byte boundary, through the C ABI
# ---------------------------------------------------------------------------
def _c_calls(dev):
    from dmesh_renderer_amd import _C
    return declare(C.CDLL(_C.library_path()), ["dmr_hashgrid_rows", "dmr_hashgrid_rows_backward"])


@pytest.mark.parametrize("i", range(len(HC.MISALIGNED)))
def test_y_one_float_off_a_16_byte_boundary(hip_device, i):
    """The same call with y, grad_out and dL_dx at base + 4 bytes: the forward bit-equal, the gradients within sum_order_tol;
    the words around the three buffers unchanged."""
    c, dev = HC.MISALIGNED[i], hip_device
    d, spec, lib = _inputs(c), _spec(c), _c_calls(hip_device)
    C_, stream = c.L * c.F, th.cuda.current_stream(dev).cuda_stream
    x, table, up = d["x"].to(dev), d["table"].to(dev), d["up_x"].to(dev)
    res = (C.c_int32 * c.L)(*spec.resolutions)
    outs = []
    for off in (0, 1):
        (ybuf, y), (gbuf, g), (dxbuf, dx) = (guarded(dev, c.N * w, off) for w in (C_, C_, 3))
        g.copy_(up.flatten())
        dt = th.full_like(table, float("nan"))
        with th.cuda.device(dev):
            assert lib.dmr_hashgrid_rows(c.N, c.L, c.F, c.log2_T, res, x.data_ptr(), table.data_ptr(), None, y.data_ptr(), stream) == 0, lib.dmr_last_error()
            assert lib.dmr_hashgrid_rows_backward(c.N, c.L, c.F, c.log2_T, res, x.data_ptr(), table.data_ptr(), None, g.data_ptr(), dx.data_ptr(),
                                                  dt.data_ptr(), stream) == 0, lib.dmr_last_error()
        th.cuda.synchronize()
        assert all(intact(buf, c.N * w, off) for buf, w in ((ybuf, C_), (gbuf, C_), (dxbuf, 3)))   # every sentinel word on both sides
        outs.append((y.cpu().numpy().reshape(c.N, C_), dx.cpu().numpy().reshape(c.N, 3), dt.cpu().numpy()))
    (y0, dx0, dt0), (y1, dx1, dt1) = outs
    e_x, e_t = rel_err(dx1, dx0), rel_err(dt1, dt0)
    print(f"\n{c}: y equal {np.array_equal(y0, y1)}, dL_dx {e_x:.2e}, dL_dtable {e_t:.2e} from the aligned call")
    assert np.array_equal(y0, y1) and e_x <= sum_order_tol("x") and e_t <= sum_order_tol("table")
    ref, bounds = _models(c)
    for k, got in (("y", y1), ("x", dx1), ("tx", dt1)):
        assert rel_err(got, ref[k]) <= bounds[k][0], k


# ---------------------------------------------------------------------------
# Special coordinates
# ---------------------------------------------------------------------------
def test_special_coordinates(hip_device):
    """Coordinates exactly 0 and 1, on grid vertices, at -0.5, 1.5, +-Inf, NaN and 1e30: y and the gradients are finite and equal
    the model's (the resolutions are powers of two: p = u R is exact, so float32 and float64 agree on every cell and no row is left
    out), dL/dx an exact 0 on the clamped and NaN coordinates."""
    c, inf, nan = HC.SPECIAL, float("inf"), float("nan")
    spec = _spec(c)
    assert spec.resolutions == (4, 8, 16, 32) and spec.sizes == (125, 729, 1024, 1024)
    rows = [[0, 0, 0], [1, 1, 1], [0, 1, 0.5], [0.25, 0.5, 0.75], [3 / 32, 17 / 32, 1], [0.3, 0.6, 0.9], [-0.5, 0.3, 0.6], [0.2, 1.5, 0.4],
            [inf, 0.3, 0.3], [0.4, -inf, 0.3], [0.7, 0.1, nan], [nan, nan, nan], [1e30, -1e30, 0.55], [inf, -inf, nan], [0.999, 0.001, 0.5]]
    x = th.tensor(rows, dtype=th.float32).repeat(9, 1)   # 135 rows: three waves, the special rows in every one
    outside = ~((x >= 0) & (x <= 1))
    g = th.Generator().manual_seed(11)
    table, up = th.randn(spec.offsets[-1], c.F, generator=g), th.randn(len(x), c.L * c.F, generator=g)
    res = []
    for f, dev, dtype in ((FG.hashgrid_rows_fused, hip_device, th.float32), (FG.hashgrid_rows, "cpu", th.float64)):
        xx, tt = x.to(dev, dtype).requires_grad_(True), table.to(dev, dtype).requires_grad_(True)
        y = f(xx, tt, spec)
        gx, gt = th.autograd.grad(y, [xx, tt], grad_outputs=up.to(dev, dtype))
        res.append([t.detach().cpu().numpy() for t in (y, gx, gt)])
    for k, a, b in zip(("y", "x", "table"), *res):
        e = rel_err(a, b)
        print(f"\nspecial coordinates {k}: {e:.2e} (max |ref| {float(np.abs(b).max()):.3g})")
        assert np.isfinite(a).all() and np.isfinite(b).all() and e <= (FWD_TOL if k == "y" else GRAD_TOL), (k, e)
    gx = res[0][1]
    assert float(np.abs(gx[outside.numpy()]).max()) == 0.0 and float(np.abs(res[1][1][outside.numpy()]).max()) == 0.0
    assert float(np.abs(gx[~outside.numpy()]).min()) > 0   # ... and exactly 0 and 1 pass


# ---------------------------------------------------------------------------
# n_rows
# ---------------------------------------------------------------------------
def test_n_rows_on_the_device(hip_device):
    """The counts 0, below N, N, above N and negative, NaN in the tail rows of x and of the upstream: exact zeros in the tails of y
    and dL_dx, dL_dtable equal to the truncated call's."""
    c = HC.N_ROWS
    base = _inputs(c)
    for n in n_rows_counts(c.N):
        m = min(max(n, 0), c.N)
        d = dict(base, x=base["x"].clone(), up=base["up"].clone(), up_x=base["up_x"].clone())
        d["x"][m:], d["up"][m:], d["up_x"][m:] = float("nan"), float("nan"), float("nan")
        got = _run(FG.hashgrid_rows_fused, c, d, hip_device, th.float32, n)
        clean = {k: (th.nan_to_num(v) if isinstance(v, th.Tensor) else v) for k, v in d.items()}
        ref = _run(FG.hashgrid_rows, c, clean, "cpu", th.float64, n)
        within_floors(f"n_rows {n} of {c.N},", ref, got, rel_err)
        assert float(np.abs(got["y"][m:]).sum()) == 0.0 and float(np.abs(got["x"][m:]).sum()) == 0.0
        assert m == 0 or (float(np.abs(got["y"][:m]).max()) > 0 and float(np.abs(got["x"][:m]).max()) > 0)
        if m == 0:
            assert all(float(np.abs(got[k]).max()) == 0.0 for k in got)
        else:   # the truncated call: the first m rows alone, no n_rows
            cut = c._replace(N=m)
            short = _run(FG.hashgrid_rows_fused, cut, {k: (v[:m] if isinstance(v, th.Tensor) and k != "table" else v) for k, v in clean.items()},
                         hip_device, th.float32)
            e = rel_err(got["t"], short["t"])
            print(f"\nn_rows {n} of {c.N}: dL_dtable {e:.2e} from the truncated call")
            assert e <= sum_order_tol("table") and np.array_equal(got["y"][:m], short["y"]) and np.array_equal(got["x"][:m], short["x"])


# ---------------------------------------------------------------------------
# Gradient subsets
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(HC.ONLY)))
def test_only_what_is_asked(hip_device, i):
    """Each gradient asked alone equals the pair's (dL_dx bit for bit, dL_dtable within sum_order_tol) and the model's; no
    upstream gives Nones."""
    c = HC.ONLY[i]
    d = _inputs(c)
    pair = _run(FG.hashgrid_rows_fused, c, d, hip_device, th.float32)
    _check(str(c), c, pair)
    only_x = _run(FG.hashgrid_rows_fused, c, d, hip_device, th.float32, want="x")
    only_t = _run(FG.hashgrid_rows_fused, c, d, hip_device, th.float32, want="t")
    spec = _spec(c)
    x, table = d["x"].to(hip_device).requires_grad_(True), d["table"].to(hip_device).requires_grad_(True)
    tx, = th.autograd.grad(FG.hashgrid_rows_fused(x.detach(), table, spec), [table], grad_outputs=d["up_x"].to(hip_device))
    e_t, e_tx = rel_err(only_t["t"], pair["t"]), rel_err(tx.cpu().numpy(), pair["tx"])
    print(f"\n{c}: only dL_dx equal {np.array_equal(only_x['x'], pair['x'])}; only dL_dtable {e_t:.2e} / {e_tx:.2e} from the pair's")
    assert np.array_equal(only_x["x"], pair["x"]) and e_t <= sum_order_tol("table") and e_tx <= sum_order_tol("table")
    _check(str(c) + " alone", c, dict(only_x, **only_t))
    y = FG.hashgrid_rows_fused(x, table, spec)
    assert y.requires_grad
    assert all(g is None for g in th.autograd.grad((x * 2).sum() + 0 * y.detach().sum(), [table], allow_unused=True))
    assert not FG.hashgrid_rows_fused(x.detach(), table.detach(), spec).requires_grad


def test_no_upstream_launches_nothing(hip_device, monkeypatch):
    """An output the loss does not use reaches the Function's backward as None: Nones go down and the binding is not called."""
    from dmesh_renderer_amd import _C
    c = HC.ONLY[1]
    d, spec = _inputs(c), _spec(c)
    x, table = d["x"].to(hip_device).requires_grad_(True), d["table"].to(hip_device).requires_grad_(True)
    y = FG.hashgrid_rows_fused(x, table, spec)
    z = y * 1.0
    calls = counts_calls(monkeypatch, _C, "hashgrid_rows_backward")
    grads = th.autograd.grad((x * 3).sum(), [x, table], allow_unused=True)
    assert grads[1] is None and not calls
    assert FG._HashGridRowsFn.backward(y.grad_fn, None) == (None, None, None, None) and not calls
    th.autograd.grad(z.sum(), [table])
    assert calls == [1]


# ---------------------------------------------------------------------------
# The chain on rendered lists
# ---------------------------------------------------------------------------
def _chain(dev, r, t, args, name, K):
    """pack_slots_fused -> interpolate_packed_fused (hit points) -> HashGrid -> RowMLP -> composite_values_packed_fused on a
    renderer's lists (fragment_grads=True, capacity=M) against the same chain with fragments.hashgrid_rows and mlp_rows in the
    middle, on the device: the image, table.grad, the MLP's gradients and verts.grad -- the path through dL/dx and frag.bary."""
    F = t["faces"].shape[0]
    th.manual_seed(4)
    lo, hi = t["verts"].min(0).values - 0.01, t["verts"].max(0).values + 0.01
    kw = {k: v for k, v in HC.CHAIN.items() if k != "hidden"}
    grid = FG.HashGrid(lo=lo.tolist(), hi=hi.tolist(), **kw).to(dev)
    with th.no_grad():
        grid.table.normal_()   # (the initialisation's 1e-4 would leave the MLP nothing to see)
    mlp = FG.RowMLP(grid.out_features, HC.CHAIN["hidden"], 3, activation="relu", out_activation="sigmoid").to(dev)
    params = [grid.table] + list(mlp.parameters())
    g_image, res = None, []
    for fused in (True, False):
        verts = t["verts"].clone().requires_grad_(True)
        frag = r(*(verts if k == "verts" else t[k] for k in args))[-1]
        packed = FG.pack_slots_fused(frag, F, frag.pix_to_face.numel())
        n_rows = packed.n_used
        hit = FG.interpolate_packed_fused(frag, packed, t["faces"], verts)
        if fused:
            rgb = mlp(grid(hit, n_rows=n_rows), n_rows=n_rows)
        else:
            u = (hit - grid.lo) / (grid.hi - grid.lo)
            rgb = FG.mlp_rows(FG.hashgrid_rows(u, grid.table, grid.spec, n_rows), list(mlp.weights), list(mlp.biases), activation=mlp.activation,
                              out_activation=mlp.out_activation, n_rows=n_rows)
        image, T = FG.composite_values_packed_fused(frag, packed, t["faces_opacity"], rgb)
        if g_image is None:
            g_image = th.randn(image.shape, generator=th.Generator().manual_seed(6)).to(dev)
        grads = th.autograd.grad((image * g_image).sum(), [verts] + params)
        res.append([image.detach().cpu().numpy()] + [g.cpu().numpy() for g in grads])
        used = int(packed.n_used)
    names = ["image", "verts", "table"] + [f"w{l}" for l in range(len(mlp.weights))] + [f"b{l}" for l in range(len(mlp.weights))]
    for k, a, b in zip(names, *res):
        e = rel_err(a, b)
        print(f"\n{name} ({used} rows of {packed.rows}): {k} {e:.2e} (max |ref| {float(np.abs(b).max()):.3g})")
        assert float(np.abs(b).max()) > 0 and float(np.abs(a).max()) > 0 and e <= (FWD_TOL if k == "image" else GRAD_TOL), (name, k, e)


def test_chain_on_rendered_tri_lists(hip_device):
    import dmesh_renderer_amd as dmr
    dev, K, Hs, Ws = hip_device, 4, 80, 112
    t = {k: v.to(dev) for k, v in scenes.layered_sheets(4, 8, 1, Hs, Ws, seed=3, opacity=(0.1, 0.4)).items()}
    r = dmr.TriRenderer(dmr.TriRenderSettings(Hs, Ws, t["bg"]), return_fragments=K, fragment_grads=True)
    _chain(dev, r, t, TRI_ARGS, "tri", K)


def test_chain_on_rendered_tet_lists(hip_device):
    import dmesh_renderer_amd as dmr
    dev, K, Hs, Ws = hip_device, 4, 48, 72
    t = {k: v.to(dev) for k, v in scenes.kuhn_tets(2, 1, Hs, Ws, seed=5).items()}
    r = dmr.TetRenderer(dmr.TetRenderSettings(Hs, Ws, t["bg"], 0), return_fragments=K, fragment_grads=True)
    _chain(dev, r, t, TET_ARGS, "tet", K)


# ---------------------------------------------------------------------------
# Graph replay
# ---------------------------------------------------------------------------
def test_graph_replay(hip_device):
    """Forward + backward with n_rows on the device, captured into one HIP graph and replayed over x, table and n_rows rewritten
    in place, the count going down and up: the stored outputs (y, dL_dx) equal the eager ones, dL_dtable is within sum_order_tol,
    the tail rows are exact zeros, and so is every table row no point touched -- on every replay (the zeroing is a kernel)."""
    dev, c = hip_device, HC.GRAPH
    d, spec = _inputs(c), _spec(c)
    x = d["x"].to(dev).requires_grad_(True)
    table = d["table"].to(dev).requires_grad_(True)
    up, n_rows = d["up"].to(dev), th.tensor([500], dtype=th.int32, device=dev)
    names = ["y", "x", "table"]

    def step():
        y = FG.hashgrid_rows_fused(x, table, spec, n_rows)
        return [y.detach()] + list(th.autograd.grad(y, [x, table], grad_outputs=up))

    def touched():
        """bool [rows]: the table rows the first n_rows points read (the model's gradient of sum(y) is non-zero exactly there)."""
        ones = th.ones(table.shape, requires_grad=True)   # float32 on the CPU: the kernels' cells and weights (all >= 0: no cancellation)
        FG.hashgrid_rows(x.detach().cpu()[:int(n_rows)], ones, spec).sum().backward()
        return (ones.grad.abs().sum(1) > 0).to(dev)

    def same(captured, eager, what):
        n = int(n_rows)
        for k, a, b in zip(names, captured, eager):
            if k in ("y", "x"):
                print(f"\ngraph replay vs eager, {what}, {k}: equal {th.equal(a, b)}")
                assert th.equal(a, b), (what, k)
                assert float(a[n:].abs().sum()) == 0.0 and float(a[:n].abs().max()) > 0
            else:
                e = rel_err(a.cpu().numpy(), b.cpu().numpy())
                hit = touched()
                print(f"\ngraph replay vs eager, {what}, {k}: {e:.2e} (max |eager| {float(b.abs().max()):.3g}); {int(hit.sum())} of {len(hit)} rows touched")
                assert float(b.abs().max()) > 0 and e <= sum_order_tol(k), (what, k, e)
                assert 0 < int(hit.sum()) < len(hit) and float(a[~hit].abs().sum()) == 0.0

    graph, captured, eager = capture_replay(step)
    for t in captured:
        t.fill_(1)
    replay(graph)
    same(captured, eager, "the captured inputs")
    g = th.Generator().manual_seed(9)
    for n in (90, c.N):
        with th.no_grad():
            x.copy_(th.rand(c.N, 3, generator=g).to(dev))
            table.copy_(th.randn(table.shape, generator=g).to(dev))
            n_rows.fill_(n)
        replay(graph)
        fresh = [t.detach().clone() for t in step()]
        th.cuda.synchronize()
        same(captured, fresh, f"x, table and n_rows = {n} rewritten in place")
