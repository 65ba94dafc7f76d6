"""fragments.sh_rows_fused, packed_row_views_fused and ViewSH on the GPU (csrc/dmr_sh.hip: k_sh_rows, k_sh_rows_backward,
k_sh_row_views; csrc/dmr_rows_common.hip: k_rows_fill) against fragments.sh_rows / packed_row_views evaluated in float64 on the CPU, on the same float32
inputs cast up: the case table of tests/sh_cases.py (every instantiation; N around a wave, a workgroup's tile and the capped
grid; B = 1, 2, 5; rows of one view, views changing inside a wave, exactly at wave and workgroup edges, shuffled, with -1 and
>= B scattered in; origin=None and origin [1,3]), x and y off a 16-byte boundary, special rows, n_rows on the device, single
gradients, the row-to-view map on the packed unit's shapes, the ray directions of rendered lists, the chain pack -> hit points
-> HashGrid + ViewSH -> RowMLP -> blend on rendered lists, and a replayed HIP graph.

Inputs: |x - origin[view]| in [0.5, 3], upstream ~ N(0,1).  Errors are max |got - ref| / max |ref| (_rel, which is
row_units.rel_to_largest).  Bounds (the project's own): y within max(FWD_TOL = 1e-5, 4 x the yardstick), gradients within
max(GRAD_TOL = 1e-4, 4 x the yardstick), the yardstick being fragments.sh_rows in float32 on the CPU against float64 on the same case; never
anything the kernels gave.  Every case prints what it measured (pytest -s).

MEASURED on the MI355X, the largest figure over the table's 32 cases (in brackets float32 torch on the CPU on the same cases, the
yardstick): y 4.0e-7 (4.5e-7), dL_dx 2.6e-7 (3.4e-7), dL_dorigin 1.8e-6 (9.1e-6).  The 4 misaligned calls give the aligned calls'
y, dL_dx and dL_dorigin bit for bit.  Special rows: y 3.1e-7, dL_dx 2.5e-7, dL_dorigin 1.3e-7, exact zeros in the special rows.
n_rows: at most 3.4e-7.  A single gradient alone: equal to the pair's.  packed_row_views_fused: equal on 8 shapes x 5 capacities
(up to 165 366 used slots).  Ray directions on 3 685 interior slots of two views: fused 1.9e-7, float32 torch 1.9e-7.  The chains
(tri 15 795 rows of 59 904 with capacity=M; tet 9 630 of 23 936): image 6.0e-8, verts.grad 3.1e-7, mv_mats.grad 1.5e-6, table.grad
5.2e-8, the MLP's gradients to 3.7e-6.  Graph replays against eager (n_rows 500 -> 90 -> 700 of 700 rows): y, dL_dx and dL_dorigin
equal, dL_dorigin 2.0e-7 from float64, exact zeros in the rows that are not read.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch as th

import sh_cases as SC
import dmesh_renderer_amd as dmr
from dmesh_renderer_amd import fragments as FG
from dmesh_renderer_amd import scenes
from harness import TET_ARGS, TRI_ARGS, capture_replay, replay
from row_units import FWD_TOL, GRAD_TOL, check, counts_calls, declare, guarded, intact, models, n_rows_counts, within_floors
from row_units import rel_to_largest as _rel
from tri_grad_ref import pixel_rays
from util import rel_err, sum_order_tol

pytestmark = pytest.mark.gpu

C0 = 0.28209479177387814


@functools.lru_cache(maxsize=None)
def _inputs(c, seed=0):
    """float32 / int32 CPU tensors of a case: x, origin, row_view and the upstream."""
    x, origin = SC.rows_of(c, seed)
    g = th.Generator().manual_seed(1000 * seed + 7 * c.N + 13 * c.degree + c.B)
    return dict(x=th.from_numpy(x), origin=th.from_numpy(origin), view=th.from_numpy(SC.views_of(c, seed)),
                up=th.randn(c.N, c.degree ** 2, generator=g))


def _run(f, c, d, device, dtype, n=None, want=None):
    """{"y", "x" (dL/dx), "o" (dL/dorigin)} of one call as numpy; n: the n_rows count or None; want: c.want unless given."""
    want = want or c.want
    x = d["x"].clone().to(device, dtype).requires_grad_("x" in want)       # (clones: on the CPU in float32 .to() is the cached tensor itself)
    origin = None if c.form == "dirs" else d["origin"].clone().to(device, dtype).requires_grad_("o" in want)
    view = d["view"].to(device) if c.form == "views" else None
    nr = None if n is None else th.tensor([n], dtype=th.int32, device=device)
    y = f(x, c.degree, origin=origin, row_view=view, n_rows=nr)
    out = {"y": y.detach().cpu().numpy()}
    leaves = [t for k, t in (("x", x), ("o", origin)) if k in want]
    grads = th.autograd.grad(y, leaves, grad_outputs=d["up"].to(device, dtype))
    out.update({k: g.cpu().numpy() for k, g in zip([k for k in "xo" if k in want], grads)})
    return out


@functools.lru_cache(maxsize=None)
def _models(c, n=None):
    """fragments.sh_rows on the CPU in float64 and in float32 -> (reference, {name: (the bound of the case, the yardstick)})."""
    return models(_run, FG.sh_rows, c, _inputs(c), n, _rel)


def _check(what, c, got, n=None):
    return check(what, *_models(c, n), got, _rel)


@pytest.mark.parametrize("i", range(len(SC.TABLE)))
def test_table(hip_device, i):
    c = SC.TABLE[i]
    d = _inputs(c)
    got = _run(FG.sh_rows_fused, c, d, hip_device, th.float32)
    ref = _check(str(c), c, got)
    if c.N == 0:
        assert ref["y"].shape == (0, c.degree ** 2) and float(np.abs(got["o"]).max()) == 0.0
        return
    assert float(np.abs(ref["y"]).max()) > 0 and (c.degree == 1 or float(np.abs(ref["x"]).max()) > 0)
    if c.form == "views":   # rows without a view: exact zeros, channel 0 included
        skipped = (d["view"].numpy() < 0) | (d["view"].numpy() >= c.B)
        assert float(np.abs(got["y"][skipped]).sum()) == 0.0 and float(np.abs(got["x"][skipped]).sum()) == 0.0
        assert (got["y"][~skipped, 0] == np.float32(C0)).all()
    if c.degree == 1:
        assert all(float(np.abs(got[k]).max()) == 0.0 for k in got if k != "y")   # a constant: exact zeros


# ---------------------------------------------------------------------------
# x, y (and the upstream, dL_dx) one float off a 16-byte boundary, through the C ABI
# ---------------------------------------------------------------------------
def _c_calls():
    from dmesh_renderer_amd import _C
    return declare(C.CDLL(_C.library_path()), ["dmr_sh_rows", "dmr_sh_rows_backward"])


@pytest.mark.parametrize("i", range(len(SC.MISALIGNED)))
def test_one_float_off_a_16_byte_boundary(hip_device, i):
    """The same call with x, y, grad_out and dL_dx at base + 4 bytes: y and dL_dx bit-equal, dL_dorigin within sum_order_tol;
    the words around the four buffers unchanged."""
    c, dev = SC.MISALIGNED[i], hip_device
    d, lib = _inputs(c), _c_calls()
    C_, stream = c.degree ** 2, th.cuda.current_stream(dev).cuda_stream
    origin, up = d["origin"].to(dev), d["up"].to(dev)
    view = d["view"].to(dev) if c.form == "views" else None
    outs = []
    for off in (0, 1):
        (xbuf, x), (ybuf, y), (gbuf, g), (dxbuf, dx) = (guarded(dev, c.N * w, off) for w in (3, C_, C_, 3))
        x.copy_(d["x"].to(dev).flatten())
        g.copy_(up.flatten())
        do = th.full_like(origin, float("nan"))
        vp = None if view is None else view.data_ptr()
        with th.cuda.device(dev):
            assert lib.dmr_sh_rows(c.N, c.degree, c.B, x.data_ptr(), origin.data_ptr(), vp, None, y.data_ptr(), stream) == 0, lib.dmr_last_error()
            assert lib.dmr_sh_rows_backward(c.N, c.degree, c.B, x.data_ptr(), origin.data_ptr(), vp, None, g.data_ptr(), dx.data_ptr(),
                                            do.data_ptr(), stream) == 0, lib.dmr_last_error()
        th.cuda.synchronize()
        assert all(intact(buf, c.N * w, off) for buf, w in ((xbuf, 3), (ybuf, C_), (gbuf, C_), (dxbuf, 3)))   # every sentinel word on both sides
        outs.append((y.cpu().numpy().reshape(c.N, C_), dx.cpu().numpy().reshape(c.N, 3), do.cpu().numpy()))
    (y0, dx0, do0), (y1, dx1, do1) = outs
    e_o = _rel(do1, do0)
    print(f"\n{c}: y equal {np.array_equal(y0, y1)}, dL_dx equal {np.array_equal(dx0, dx1)}, dL_dorigin {e_o:.2e} from the aligned call")
    assert np.array_equal(y0, y1) and np.array_equal(dx0, dx1) and e_o <= sum_order_tol("origin")
    ref, bounds = _models(c)
    for k, got in (("y", y1), ("x", dx1), ("o", do1)):
        assert _rel(got, ref[k]) <= bounds[k][0], k


# ---------------------------------------------------------------------------
# Special rows
# ---------------------------------------------------------------------------
def test_special_rows(hip_device):
    """x == origin exactly, NaN, +-Inf and 1e30 rows: the zero direction (channel 0 alone), exact-zero dL/dx, nothing added to
    dL/dorigin, everything finite; the rows between them (|w| >= 0.1) are the model's.  The float64 reference holds x = origin[v]
    in the special rows: in float64 1e30 has a direction, in the tensor's own dtype |w|^2 overflows."""
    dev, nan, inf = hip_device, float("nan"), float("inf")
    g = th.Generator().manual_seed(21)
    B, N = 2, 192   # three waves, the special rows in every one
    origin = th.rand(B, 3, generator=g) * 4 - 2
    view = (th.arange(N) // 40 % B).to(th.int32)
    d = th.randn(N, 3, generator=g)
    x = origin[view.long()] + d / d.norm(dim=1, keepdim=True) * (0.1 + 2.9 * th.rand(N, 1, generator=g))
    special = th.zeros(N, dtype=th.bool)
    for k, row in enumerate(([0, 0, 0], [nan, 0.3, 0.2], [inf, 0.0, 1.0], [0.1, -inf, nan], [1e30, 0.0, 0.0], [-1e30, 1e30, 1e30], [nan, nan, nan])):
        for wave in range(3):
            r = 64 * wave + 9 * k + wave
            x[r] = origin[view[r]] if k == 0 else th.tensor(row)
            special[r] = True
    up = th.randn(N, 16, generator=g)
    xr = th.where(special.unsqueeze(1), origin[view.long()], x)
    res = []
    for f, device, dtype, xx in ((FG.sh_rows_fused, dev, th.float32, x), (FG.sh_rows, "cpu", th.float64, xr)):
        a, o = xx.to(device, dtype).requires_grad_(True), origin.to(device, dtype).requires_grad_(True)
        y = f(a, 4, origin=o, row_view=view.to(device))
        gx, go = th.autograd.grad(y, [a, o], grad_outputs=up.to(device, dtype))
        res.append([t.detach().cpu().numpy() for t in (y, gx, go)])
    for k, a, b in zip(("y", "x", "origin"), *res):
        e = _rel(a, b)
        print(f"\nspecial rows {k}: {e:.2e} (max |ref| {float(np.abs(b).max()):.3g})")
        assert np.isfinite(a).all() and e <= (FWD_TOL if k == "y" else GRAD_TOL), (k, e)
    y, gx = res[0][0], res[0][1]
    s = special.numpy()
    assert (y[s, 0] == np.float32(C0)).all() and float(np.abs(y[s, 1:]).max()) == 0.0 and float(np.abs(gx[s]).max()) == 0.0
    assert float(np.abs(gx[~s]).max(1).min()) > 0


# ---------------------------------------------------------------------------
# n_rows
# ---------------------------------------------------------------------------
def test_n_rows_on_the_device(hip_device):
    """The counts 0, below N, N, above N and negative, NaN in the tail rows of x and of the upstream: exact zeros in the tails of y
    and dL_dx, dL_dorigin the model's."""
    c = SC.N_ROWS
    base = _inputs(c)
    for n in n_rows_counts(c.N):
        m = min(max(n, 0), c.N)
        d = dict(base, x=base["x"].clone(), up=base["up"].clone())
        d["x"][m:], d["up"][m:] = float("nan"), float("nan")
        got = _run(FG.sh_rows_fused, c, d, hip_device, th.float32, n)
        clean = {k: (th.nan_to_num(v) if v.dtype.is_floating_point else v) for k, v in d.items()}
        ref = _run(FG.sh_rows, c, clean, "cpu", th.float64, n)
        within_floors(f"n_rows {n} of {c.N},", ref, got, _rel)
        assert float(np.abs(got["y"][m:]).sum()) == 0.0 and float(np.abs(got["x"][m:]).sum()) == 0.0
        if m == 0:
            assert all(float(np.abs(got[k]).max()) == 0.0 for k in got)
        else:
            assert float(np.abs(got["y"][:m]).max()) > 0 and float(np.abs(got["x"][:m]).max()) > 0 and float(np.abs(got["o"]).max()) > 0


# ---------------------------------------------------------------------------
# Gradient subsets
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(SC.ONLY)))
def test_only_what_is_asked(hip_device, i):
    """Each gradient asked alone equals the pair's (dL_dx bit for bit, dL_dorigin within sum_order_tol) and the model's."""
    c = SC.ONLY[i]
    d = _inputs(c)
    pair = _run(FG.sh_rows_fused, c, d, hip_device, th.float32)
    _check(str(c), c, pair)
    only_x = _run(FG.sh_rows_fused, c, d, hip_device, th.float32, want="x")
    only_o = _run(FG.sh_rows_fused, c, d, hip_device, th.float32, want="o")
    e_o = _rel(only_o["o"], pair["o"])
    print(f"\n{c}: only dL_dx equal {np.array_equal(only_x['x'], pair['x'])}; only dL_dorigin {e_o:.2e} from the pair's")
    assert set(only_x) == {"y", "x"} and set(only_o) == {"y", "o"}
    assert np.array_equal(only_x["x"], pair["x"]) and np.array_equal(only_x["y"], pair["y"]) and e_o <= sum_order_tol("origin")
    _check(str(c) + " alone", c, dict(only_x, **only_o))
    x, origin = d["x"].to(hip_device), d["origin"].to(hip_device)
    assert not FG.sh_rows_fused(x, c.degree, origin=origin, row_view=d["view"].to(hip_device)).requires_grad


def test_no_upstream_launches_nothing(hip_device, monkeypatch):
    """An output the loss does not use reaches the Function's backward as None: Nones go down and the binding is not called."""
    from dmesh_renderer_amd import _C
    c = SC.ONLY[3]
    d = _inputs(c)
    x, origin = d["x"].to(hip_device).requires_grad_(True), d["origin"].to(hip_device).requires_grad_(True)
    y = FG.sh_rows_fused(x, c.degree, origin=origin, row_view=d["view"].to(hip_device))
    z = y * 1.0
    calls = counts_calls(monkeypatch, _C, "sh_rows_backward")
    grads = th.autograd.grad((x * 3).sum(), [x, origin], allow_unused=True)
    assert grads[1] is None and not calls
    assert FG._ShRowsFn.backward(y.grad_fn, None) == (None, None, None, None, None) and not calls
    th.autograd.grad(z.sum(), [origin])
    assert calls == [1]


# ---------------------------------------------------------------------------
# Which view a row belongs to
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(SC.VIEW_SHAPES)))
def test_packed_row_views(hip_device, i):
    """packed_row_views_fused equals the model exactly, with an exact pack and with capacities 0, below, at and above the count."""
    B, K, H, W, share = SC.VIEW_SHAPES[i]
    g = th.Generator().manual_seed(31 + i)
    F = 40
    face = th.where(th.rand(B, K, H, W, generator=g) < share, th.randint(0, F, (B, K, H, W), generator=g), th.full((B, K, H, W), -1)).to(th.int32)
    used = int((face >= 0).sum())
    frag = dmr.Fragments(face.to(hip_device), None, None)
    for capacity in (None, 0, used // 2, used, used + 77):
        packed = FG.pack_slots_fused(frag, F, capacity)
        got = FG.packed_row_views_fused(frag, packed)
        want = FG.packed_row_views(dmr.Fragments(face, None, None), FG.PackedSlots(packed.row.cpu(), packed.n_used.cpu(), packed.rows))
        assert got.dtype == th.int32 and tuple(got.shape) == (packed.rows,) and th.equal(got.cpu(), want), (SC.VIEW_SHAPES[i], capacity)
        n = min(used, packed.rows)
        assert bool((got[:n] >= 0).all()) and bool((got[n:] == -1).all())
    print(f"\n{SC.VIEW_SHAPES[i]}: {used} used slots, equal at every capacity")


# ---------------------------------------------------------------------------
# Rendered lists: the direction of a packed row is its pixel's ray
# ---------------------------------------------------------------------------
def test_directions_of_rendered_tri_lists_are_the_pixel_rays(hip_device):
    """Two views with different cameras, fragment lists with barycentrics.  On slots strictly inside their face the hit point lies
    on the pixel's ray, so normalize(hit - camera_origins(mv)[view]) -- read back from channels 1..3 of the fused encoding -- is
    the ray direction, computed here in float64 from the inverse matrices by pixel_ray's arithmetic (tests/tri_grad_ref.py).  The
    bound is 4 x what the float32 torch path (interpolate_packed + sh_rows on the device) gives on the same lists; a wrong
    camera_origins or a wrong row-to-view map misses it by orders of magnitude (the two cameras face each other)."""
    dev, K, Hs, Ws = hip_device, 4, 40, 56
    t = {k: v.to(dev) for k, v in scenes.layered_sheets(3, 6, 2, Hs, Ws, seed=7, opacity=(0.1, 0.4)).items()}
    r = dmr.TriRenderer(dmr.TriRenderSettings(Hs, Ws, t["bg"]), return_fragments=K, fragment_grads=True)
    frag = r(*(t[k] for k in TRI_ARGS))[-1]
    F = t["faces"].shape[0]
    packed = FG.pack_slots_fused(frag, F)
    origin = FG.camera_origins(t["mv_mats"])
    assert float((origin[0] - origin[1]).norm()) > 1
    c1 = 0.4886025119029199

    def directions(fused):
        if fused:
            view = FG.packed_row_views_fused(frag, packed)
            y = FG.sh_rows_fused(FG.interpolate_packed_fused(frag, packed, t["faces"], t["verts"]), 2, origin=origin, row_view=view)
        else:
            view = FG.packed_row_views(frag, packed)
            y = FG.sh_rows(FG.interpolate_packed(frag, packed, t["faces"], t["verts"]), 2, origin=origin, row_view=view)
        return th.stack([-y[:, 3], -y[:, 1], y[:, 2]], 1).double().cpu() / c1, view.cpu()

    u, v = frag.bary[:, :, 0].detach().cpu(), frag.bary[:, :, 1].detach().cpu()
    row = packed.row.cpu()
    interior = (row >= 0) & (u > 1e-3) & (v > 1e-3) & (u + v < 1 - 1e-3)
    b, k, py, px = interior.nonzero(as_tuple=True)
    rows = row[interior].long()
    _, ray = pixel_rays(t["mv_mats"].double().cpu(), t["proj_mats"].double().cpu(), b, px, py, Hs, Ws)
    ray = ray / ray.norm(dim=1, keepdim=True)
    (got, view), (f32, view32) = directions(True), directions(False)
    assert th.equal(view, view32) and th.equal(view[rows].long(), b)
    e, yard = float((got[rows] - ray).abs().max()), float((f32[rows] - ray).abs().max())
    print(f"\nray directions on {len(rows)} interior slots of {packed.rows} rows ({int((b == 0).sum())} / {int((b == 1).sum())} per view): "
          f"fused {e:.2e}, float32 torch {yard:.2e}")
    assert len(rows) > 500 and int((b == 0).sum()) > 100 and int((b == 1).sum()) > 100
    assert yard < 1e-4 and e <= 4 * yard
    swapped = FG.sh_rows_fused(FG.interpolate_packed_fused(frag, packed, t["faces"], t["verts"]), 2, origin=origin.flip(0), row_view=view.to(dev))
    wrong = th.stack([-swapped[:, 3], -swapped[:, 1], swapped[:, 2]], 1).double().cpu() / c1
    assert float((wrong[rows] - ray).abs().max()) > 0.1   # the other view's origin: the check above would fail


# ---------------------------------------------------------------------------
# The chain on rendered lists
# ---------------------------------------------------------------------------
def _chain(dev, r, t, args, name):
    """pack_slots_fused -> packed_row_views_fused, interpolate_packed_fused (hit points) -> HashGrid + ViewSH(4) -> RowMLP(48, 64, 3)
    -> composite_values_packed_fused on a renderer's lists (two views, fragment_grads=True, capacity=M), as the module docstring's
    example writes it, against the same chain with fragments.hashgrid_rows, sh_rows and mlp_rows in the middle, on the device:
    the image, verts.grad, table.grad, the MLP's gradients and mv_mats.grad through camera_origins."""
    F = t["faces"].shape[0]
    th.manual_seed(4)
    lo, hi = t["verts"].min(0).values - 0.01, t["verts"].max(0).values + 0.01
    kw = {k: v for k, v in SC.CHAIN.items() if k not in ("hidden", "degree")}
    grid = FG.HashGrid(lo=lo.tolist(), hi=hi.tolist(), **kw).to(dev)
    with th.no_grad():
        grid.table.normal_()   # (the initialisation's 1e-4 would leave the MLP nothing to see)
    sh = FG.ViewSH(SC.CHAIN["degree"])
    mlp = FG.RowMLP(grid.out_features + sh.out_features, SC.CHAIN["hidden"], 3, activation="relu", out_activation="sigmoid").to(dev)
    assert grid.out_features + sh.out_features == 48
    params = [grid.table] + list(mlp.parameters())
    faces, faces_opacity = t["faces"], t["faces_opacity"]
    g_image, res = None, []
    for fused in (True, False):
        verts = t["verts"].clone().requires_grad_(True)
        mv_mats = t["mv_mats"].clone().requires_grad_(True)
        frag = r(*(verts if k == "verts" else t[k] for k in args))[-1]
        packed = FG.pack_slots_fused(frag, F, frag.pix_to_face.numel())
        n = packed.n_used
        if fused:
            view = FG.packed_row_views_fused(frag, packed)
            hit = FG.interpolate_packed_fused(frag, packed, faces, verts)
            enc = th.cat([grid(hit, n_rows=n), FG.ViewSH(4)(hit, FG.camera_origins(mv_mats), view, n_rows=n)], 1)
            image, T = FG.composite_values_packed_fused(frag, packed, faces_opacity, mlp(enc, n_rows=n))
        else:
            view = FG.packed_row_views(frag, packed)
            hit = FG.interpolate_packed_fused(frag, packed, faces, verts)
            u = (hit - grid.lo) / (grid.hi - grid.lo)
            enc = th.cat([FG.hashgrid_rows(u, grid.table, grid.spec, n), FG.sh_rows(hit, 4, origin=FG.camera_origins(mv_mats), row_view=view, n_rows=n)], 1)
            rgb = FG.mlp_rows(enc, list(mlp.weights), list(mlp.biases), activation=mlp.activation, out_activation=mlp.out_activation, n_rows=n)
            image, T = FG.composite_values_packed_fused(frag, packed, faces_opacity, rgb)
        if g_image is None:
            g_image = th.randn(image.shape, generator=th.Generator().manual_seed(6)).to(dev)
        grads = th.autograd.grad((image * g_image).sum(), [verts, mv_mats] + params)
        res.append([image.detach().cpu().numpy()] + [g.cpu().numpy() for g in grads])
        used = int(packed.n_used)
    names = ["image", "verts", "mv_mats", "table"] + [f"w{l}" for l in range(len(mlp.weights))] + [f"b{l}" for l in range(len(mlp.weights))]
    for k, a, b in zip(names, *res):
        e = rel_err(a, b)
        print(f"\n{name} ({used} rows of {packed.rows}): {k} {e:.2e} (max |ref| {float(np.abs(b).max()):.3g})")
        assert float(np.abs(b).max()) > 0 and float(np.abs(a).max()) > 0 and e <= (FWD_TOL if k == "image" else GRAD_TOL), (name, k, e)


def test_chain_on_rendered_tri_lists(hip_device):
    dev, K, Hs, Ws = hip_device, 4, 72, 104
    t = {k: v.to(dev) for k, v in scenes.layered_sheets(4, 8, 2, Hs, Ws, seed=3, opacity=(0.1, 0.4)).items()}
    r = dmr.TriRenderer(dmr.TriRenderSettings(Hs, Ws, t["bg"]), return_fragments=K, fragment_grads=True)
    _chain(dev, r, t, TRI_ARGS, "tri")


def test_chain_on_rendered_tet_lists(hip_device):
    dev, K, Hs, Ws = hip_device, 4, 44, 68
    t = {k: v.to(dev) for k, v in scenes.kuhn_tets(2, 2, Hs, Ws, seed=5).items()}
    r = dmr.TetRenderer(dmr.TetRenderSettings(Hs, Ws, t["bg"], 0), return_fragments=K, fragment_grads=True)
    _chain(dev, r, t, TET_ARGS, "tet")


# ---------------------------------------------------------------------------
# Graph replay
# ---------------------------------------------------------------------------
def test_graph_replay(hip_device):
    """Forward + backward over capacity=M rows (n_rows and row_view on the device), captured into one HIP graph and replayed over
    x, origin, row_view and n_rows rewritten in place, the count going down and up: y and dL_dx equal the eager ones, dL_dorigin is
    within the gradient bound of the float64 model, and the rows that are not read -- the tail past n_rows, the rows of view -1 --
    hold exact zeros on every replay."""
    dev, c = hip_device, SC.GRAPH
    d = _inputs(c)
    x = d["x"].to(dev).requires_grad_(True)
    origin = d["origin"].to(dev).requires_grad_(True)
    view, up, n_rows = d["view"].to(dev), d["up"].to(dev), th.tensor([500], dtype=th.int32, device=dev)
    with th.no_grad():
        view[500:] = -1
    names = ["y", "x", "origin"]

    def step():
        y = FG.sh_rows_fused(x, c.degree, origin=origin, row_view=view, n_rows=n_rows)
        return [y.detach()] + list(th.autograd.grad(y, [x, origin], grad_outputs=up))

    def same(captured, eager, what):
        n = int(n_rows)
        read = (th.arange(c.N, device=dev) < n) & (view >= 0) & (view < c.B)
        a64, o64 = x.detach().double().cpu().requires_grad_(True), origin.detach().double().cpu().requires_grad_(True)
        y64 = FG.sh_rows(a64, c.degree, origin=o64, row_view=view.cpu(), n_rows=n_rows.cpu())
        ref_o = th.autograd.grad(y64, [o64], grad_outputs=up.double().cpu())[0].numpy()
        for k, a, b in zip(names, captured, eager):
            if k in ("y", "x"):
                print(f"\ngraph replay vs eager, {what}, {k}: equal {th.equal(a, b)}")
                assert th.equal(a, b), (what, k)
                assert float(a[~read].abs().sum()) == 0.0 and float(a[read].abs().max()) > 0
            else:
                e, e_ref = _rel(a.cpu().numpy(), b.cpu().numpy()), _rel(a.cpu().numpy(), ref_o)
                print(f"\ngraph replay vs eager, {what}, {k}: {e:.2e} from eager, {e_ref:.2e} from float64 (max |ref| {float(np.abs(ref_o).max()):.3g})")
                assert float(b.abs().max()) > 0 and e <= GRAD_TOL and e_ref <= GRAD_TOL, (what, k, e, e_ref)

    graph, captured, eager = capture_replay(step)
    for t in captured:
        t.fill_(1)
    replay(graph)
    same(captured, eager, "the captured inputs")
    g = th.Generator().manual_seed(9)
    for n, cut in ((90, 60), (c.N, 333)):
        with th.no_grad():
            new_origin = th.rand(c.B, 3, generator=g) * 4 - 2
            new_view = (th.arange(c.N) >= cut).to(th.int32)
            new_view[th.rand(c.N, generator=g) < 0.1] = -1
            w = th.randn(c.N, 3, generator=g)
            w = w / w.norm(dim=1, keepdim=True) * (0.5 + 2.5 * th.rand(c.N, 1, generator=g))
            x.copy_((new_origin[new_view.clamp(min=0).long()] + w).to(dev))
            origin.copy_(new_origin.to(dev))
            view.copy_(new_view.to(dev))
            n_rows.fill_(n)
        replay(graph)
        fresh = [t.detach().clone() for t in step()]
        th.cuda.synchronize()
        same(captured, fresh, f"x, origin, row_view and n_rows = {n} rewritten in place")
