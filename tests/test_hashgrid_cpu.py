"""fragments.hashgrid_spec / hashgrid_rows / hashgrid_rows_fused / HashGrid without a GPU: the torch model is an independent numpy
triple loop's numbers to 1e-12 in float64 (written from the definition, dense and hashed levels), the hash wraps modulo 2^32 at
hand-computed vertices, the dense / hashed switch sits at (R + 1)^3 == T, gradcheck passes for table and x away from cell
boundaries, dL/dx is an exact 0 on clamped and NaN coordinates, a point on a grid vertex returns that table row, the n_rows rule
is what the docstring says, HashGrid maps lo .. hi and round-trips its state_dict, dmr_hashgrid_layout equals hashgrid_spec on
every spec of the case tables, the library exports what include/dmesh_renderer_amd_hashgrid.h declares and the build lists hold
the new files, the functional layer and the C ABI refuse what the kernels do not take -- before anything reaches a device, in
their documented order -- and the case tables of the GPU tests (tests/hashgrid_cases.py) reach every kernel instantiation the
unit compiles, with at most 3 % of a case's rows in the boundary band."""
import ctypes as C
import math
import re

import numpy as np
import pytest
import torch as th

import hashgrid_cases as HC
import row_units as RU
import dmesh_renderer_amd as dmr
from dmesh_renderer_amd import fragments as FG
from row_units import D

UNIT_TEXT, HEADER_TEXT = RU.unit_texts("dmr_hashgrid.hip", "dmesh_renderer_amd_hashgrid.h")
FUNCTIONS = ["dmr_hashgrid_layout", "dmr_hashgrid_rows", "dmr_hashgrid_rows_backward"]
TORCH_PATH = r"fragments\.hashgrid_rows is the torch path"


def _spec(c):
    return FG.hashgrid_spec(c.L, c.F, c.log2_T, c.R0, c.s)


def _all_cases():
    return [c for rows in HC.tables().values() for c in rows]


# ---------------------------------------------------------------------------
# The layout
# ---------------------------------------------------------------------------
def test_spec_is_the_definition():
    s = FG.hashgrid_spec(n_levels=5, features=2, log2_table_size=12, base_resolution=3, per_level_scale=1.7)
    assert isinstance(s, FG.HashGridSpec) and s.features == 2 and s.log2_table_size == 12
    assert s.resolutions == tuple(int(math.floor(3 * 1.7 ** l)) for l in range(5)) == (3, 5, 8, 14, 25)
    assert s.sizes == (64, 216, 729, 3375, 4096)     # 4^3, 6^3, 9^3, 15^3 <= 4096 < 26^3
    assert s.offsets == (0, 64, 280, 1009, 4384, 8480)
    wide = FG.hashgrid_spec(16, 2, 19, 16, 1.38)
    assert wide.resolutions[0] == 16 and wide.resolutions[-1] == int(math.floor(16 * 1.38 ** 15)) and len(wide.offsets) == 17


def test_the_dense_hashed_switch():
    """(R + 1)^3 == T is dense; one vertex more per axis, or half the table, is hashed.  At R = 15, T = 4096 both give 4096 rows:
    the row of a vertex tells them apart."""
    at = FG.hashgrid_spec(1, 1, 12, 15, 1)
    above = FG.hashgrid_spec(1, 1, 12, 16, 1)
    below = FG.hashgrid_spec(1, 1, 11, 15, 1)
    assert at.sizes == (4096,) and above.sizes == (4096,) and below.sizes == (2048,)
    assert 16 ** 3 == 1 << 12 and 17 ** 3 == (1 << 12) + 817
    x = th.tensor([[1 / 15, 2 / 15, 3 / 15]], dtype=th.float64)

    def row_of(spec, point):
        table = th.arange(spec.offsets[-1], dtype=th.float64).unsqueeze(1)
        return float(FG.hashgrid_rows(point, table, spec)[0, 0])

    # R = 15: p = u * 15 is 1, 2, 3 up to an ulp; the vertex weights make the result the row number to 1e-9
    assert abs(row_of(at, x) - (1 + 16 * (2 + 16 * 3))) < 1e-9                      # dense: ix + 16 (iy + 16 iz) = 801
    assert abs(row_of(below, x) - ((1 ^ 1013904226 ^ 2416379583) & 2047)) < 1e-9    # hashed
    x16 = th.tensor([[1 / 16, 2 / 16, 3 / 16]], dtype=th.float64)
    assert row_of(above, x16) == ((1 ^ 1013904226 ^ 2416379583) & 4095)             # hashed although 4096 rows, like `at`


def test_hashed_rows_of_hand_computed_vertices():
    """row = (ix ^ (iy * 2654435761 mod 2^32) ^ (iz * 805459861 mod 2^32)) & (T - 1), worked by hand:
      (1, 2, 3), T = 2^14: 2 * 2654435761 = 5308871522 = 2^32 + 1013904226 (the wrap); 3 * 805459861 = 2416379583;
                           1 ^ 1013904226 ^ 2416379583 = 2892625372; & 16383 = 13788
      (5, 0, 0), T = 2^14: 5
      (0, 1, 0), T = 2^10: 2654435761 & 1023 = 433
      (3, 7, 2), T = 2^10: 7 * 2654435761 = 18581050327 = 4 * 2^32 + 1401181143; 2 * 805459861 = 1610919722;
                           3 ^ 1401181143 ^ 1610919722 = 864091390; & 1023 = 254
    R = 64 and 128 are powers of two, so the vertex coordinates i / R are exact and the result is the table row itself."""
    for (ix, iy, iz), log2_T, R, want in (((1, 2, 3), 14, 64, 13788), ((5, 0, 0), 14, 64, 5), ((0, 1, 0), 10, 128, 433), ((3, 7, 2), 10, 128, 254)):
        spec = FG.hashgrid_spec(1, 1, log2_T, R, 1)
        assert spec.sizes == (1 << log2_T,)
        table = th.arange(1 << log2_T, dtype=th.float64).unsqueeze(1)
        x = th.tensor([[ix / R, iy / R, iz / R]], dtype=th.float64)
        assert float(FG.hashgrid_rows(x, table, spec)[0, 0]) == want, (ix, iy, iz)


def test_spec_refusals_in_order():
    for kw, text in ((dict(n_levels=0), "n_levels must be in 1..16"), (dict(n_levels=17), "n_levels must be in 1..16"),
                     (dict(features=3), "features must be one of"), (dict(n_levels=16, features=8), "at most 64"),
                     (dict(log2_table_size=3), "log2_table_size must be in 4..24"), (dict(log2_table_size=25), "log2_table_size must be in 4..24"),
                     (dict(base_resolution=0), "resolution of level 0 must be in 1..65536"),
                     (dict(n_levels=14, base_resolution=16, per_level_scale=2), "resolution of level 13 must be in 1..65536"),
                     (dict(n_levels=17, features=3), "n_levels"), (dict(features=3, log2_table_size=3), "features"),
                     (dict(n_levels=16, features=8, log2_table_size=30), "at most 64"), (dict(log2_table_size=3, base_resolution=0), "log2_table_size")):
        with pytest.raises(ValueError, match="hashgrid_spec: .*" + re.escape(text)):
            FG.hashgrid_spec(**kw)
    assert FG.hashgrid_spec(13, 1, 24, 16, 2).resolutions[-1] == 65536


# ---------------------------------------------------------------------------
# The torch model against a triple loop written from the definition
# ---------------------------------------------------------------------------
def _loop_model(x, table, L, F, log2_T, R0, s):
    """y [N, L*F] in float64 by loops over rows, levels and corners; nothing shared with fragments.py."""
    T = 2 ** log2_T
    y = np.zeros((len(x), L * F))
    first = 0
    for l in range(L):
        R = int(math.floor(R0 * s ** l))
        verts = R + 1
        dense = verts ** 3 <= T
        for r in range(len(x)):
            cell, t = [], []
            for a in range(3):
                u = x[r, a]
                u = 0.0 if u != u else min(max(u, 0.0), 1.0)
                p = u * R
                i = min(int(math.floor(p)), R - 1)
                cell.append(i)
                t.append(p - i)
            for dz in (0, 1):
                for dy in (0, 1):
                    for dx in (0, 1):
                        ix, iy, iz = cell[0] + dx, cell[1] + dy, cell[2] + dz
                        if dense:
                            row = ix + verts * (iy + verts * iz)
                        else:
                            row = ((ix % 2 ** 32) ^ ((iy * 2654435761) % 2 ** 32) ^ ((iz * 805459861) % 2 ** 32)) % T
                        w = (t[0] if dx else 1 - t[0]) * (t[1] if dy else 1 - t[1]) * (t[2] if dz else 1 - t[2])
                        y[r, l * F:(l + 1) * F] += w * table[first + row]
        first += verts ** 3 if dense else T
    return y, first


def test_model_against_a_triple_loop():
    L, F, log2_T, R0, s = 6, 2, 9, 2, 1.9   # R = 2, 3, 7 dense (27, 64, 512 rows), 13, 26, 49 hashed
    spec = FG.hashgrid_spec(L, F, log2_T, R0, s)
    assert [sz == 512 for sz in spec.sizes] == [False, False, True, True, True, True] and spec.sizes[2] == 8 ** 3
    rng = np.random.default_rng(3)
    x = rng.uniform(0, 1, (50, 3))
    x[:4] = [[0, 0.5, 1], [1, 1, 1], [-0.3, 0.2, 1.4], [float("nan"), 0.7, 0.1]]
    table = rng.standard_normal((spec.offsets[-1], F))
    want, rows = _loop_model(x, table, L, F, log2_T, R0, s)
    assert rows == spec.offsets[-1]
    got = FG.hashgrid_rows(th.from_numpy(x), th.from_numpy(table), spec).numpy()
    err = float(np.abs(got - want).max())
    print(f"\nmodel against the triple loop, 50 points: {err:.2e}")
    assert got.shape == (50, L * F) and err <= 1e-12 and float(np.abs(want).max()) > 0.1


def _interior_points(n, R_finest, seed):
    """Points at least 0.05 cell away from every boundary of a level of resolution R_finest (and of the levels it refines)."""
    g = th.Generator().manual_seed(seed)
    cell = th.randint(0, R_finest, (n, 3), generator=g).double()
    return (cell + 0.05 + 0.9 * th.rand(n, 3, generator=g, dtype=th.float64)) / R_finest


def test_gradcheck():
    spec = FG.hashgrid_spec(3, 2, 6, 2, 2)   # R = 2 dense (27 rows), 4 and 8 hashed into 64 rows
    assert spec.sizes == (27, 64, 64)
    x = _interior_points(9, 8, 0).requires_grad_(True)
    table = th.randn(spec.offsets[-1], 2, dtype=th.float64, generator=th.Generator().manual_seed(1)).requires_grad_(True)
    assert th.autograd.gradcheck(lambda t: FG.hashgrid_rows(x.detach(), t, spec), (table,), eps=1e-6, atol=1e-7)
    assert th.autograd.gradcheck(lambda p: FG.hashgrid_rows(p, table.detach(), spec), (x,), eps=1e-6, atol=1e-6)
    n_rows = th.tensor([5])
    assert th.autograd.gradcheck(lambda p, t: FG.hashgrid_rows(p, t, spec, n_rows), (x, table), eps=1e-6, atol=1e-6)


def test_clamped_and_nan_coordinates_get_no_gradient():
    spec = FG.hashgrid_spec(3, 2, 6, 2, 2)
    x = th.tensor([[-0.5, 0.3, 0.6], [0.2, 1.5, 0.4], [0.7, 0.1, float("nan")], [float("inf"), float("-inf"), 1e30], [0.0, 1.0, 0.5]],
                  dtype=th.float64, requires_grad=True)
    table = th.randn(spec.offsets[-1], 2, dtype=th.float64, generator=th.Generator().manual_seed(2))
    y = FG.hashgrid_rows(x, table, spec)
    g, = th.autograd.grad(y.sum(), [x])
    assert bool(th.isfinite(y).all()) and bool(th.isfinite(g).all())
    outside = th.tensor([[1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 1], [0, 0, 0]], dtype=th.bool)
    assert float(g[outside].abs().max()) == 0.0 and float(g[~outside].abs().min()) > 0   # exactly 0 and 1 pass, as th.clamp does
    # the clamped point is the point on the face
    on_face = th.tensor([[0.0, 0.3, 0.6], [0.2, 1.0, 0.4], [0.7, 0.1, 0.0], [1.0, 0.0, 1.0]], dtype=th.float64)
    assert th.equal(y[:4].detach(), FG.hashgrid_rows(on_face, table, spec))


def test_a_point_on_a_grid_vertex_returns_that_row():
    spec = FG.hashgrid_spec(2, 4, 8, 4, 2)   # R = 4 dense (125 rows), R = 8 hashed (256 rows)
    assert spec.sizes == (125, 256)
    table = th.randn(spec.offsets[-1], 4, dtype=th.float64, generator=th.Generator().manual_seed(4))
    for v in ((0, 0, 0), (1, 3, 2), (4, 4, 4), (4, 0, 2)):   # (4, 4, 4): the upper corner, the last cell with t = 1
        x = th.tensor([[i / 4 for i in v]], dtype=th.float64)
        y = FG.hashgrid_rows(x, table, spec)[0]
        assert th.equal(y[:4], table[v[0] + 5 * (v[1] + 5 * v[2])])
        fine = [2 * i for i in v]
        row = ((fine[0] & 0xffffffff) ^ ((fine[1] * 2654435761) & 0xffffffff) ^ ((fine[2] * 805459861) & 0xffffffff)) & 255
        assert th.equal(y[4:], table[125 + row])


def test_n_rows_rule():
    spec = FG.hashgrid_spec(3, 2, 6, 2, 2)
    g = th.Generator().manual_seed(5)
    x0, table0 = th.rand(12, 3, generator=g, dtype=th.float64), th.randn(spec.offsets[-1], 2, generator=g, dtype=th.float64)
    up = th.randn(12, 6, generator=g, dtype=th.float64)
    for n, dtype in ((0, th.int32), (5, th.int64), (12, th.int32), (40, th.int32), (-3, th.int32)):
        m = min(max(n, 0), 12)
        x = x0.clone(); x[m:] = float("nan")
        u = up.clone(); u[m:] = float("nan")
        x.requires_grad_(True)
        table = table0.clone().requires_grad_(True)
        y = FG.hashgrid_rows(x, table, spec, n_rows=th.tensor([n], dtype=dtype))
        gx, gt = th.autograd.grad(y, [x, table], grad_outputs=th.nan_to_num(u))
        xs, ts = x0[:m].clone().requires_grad_(True), table0.clone().requires_grad_(True)
        ys = FG.hashgrid_rows(xs, ts, spec)
        assert bool(th.isfinite(y).all() and th.isfinite(gx).all() and th.isfinite(gt).all())
        assert th.equal(y[:m].detach(), ys.detach()) and float(y[m:].detach().abs().sum()) == 0.0 and float(gx[m:].abs().sum()) == 0.0
        if m:
            sx, st = th.autograd.grad(ys, [xs, ts], grad_outputs=up[:m])
            assert th.allclose(gx[:m], sx, rtol=0, atol=1e-12) and th.allclose(gt, st, rtol=0, atol=1e-12)
        else:
            assert float(gt.abs().sum()) == 0.0


def test_module():
    th.manual_seed(0)
    lo, hi = (-1.0, 0.0, 2.0), (1.0, 4.0, 3.0)
    grid = FG.HashGrid(n_levels=4, features=2, log2_table_size=8, base_resolution=3, per_level_scale=1.5, lo=lo, hi=hi)
    assert grid.out_features == 8 and grid.spec == FG.hashgrid_spec(4, 2, 8, 3, 1.5)
    assert tuple(grid.table.shape) == (grid.spec.offsets[-1], 2) and isinstance(grid.table, th.nn.Parameter)
    t0 = grid.table.detach()
    assert float(t0.abs().max()) <= 1e-4 and float(t0.abs().max()) > 5e-5 and float(t0.min()) < 0
    assert [n for n, _ in grid.named_parameters()] == ["table"]
    x = th.tensor([[-1.0, 0.0, 2.0], [0.0, 2.0, 2.5], [1.0, 4.0, 3.0], [5.0, -1.0, 2.25]])
    unit = th.tensor([[0.0, 0.0, 0.0], [0.5, 0.5, 0.5], [1.0, 1.0, 1.0], [3.0, -0.25, 0.25]])
    y = grid(x)
    assert tuple(y.shape) == (4, 8) and th.equal(y, FG.hashgrid_rows(unit, grid.table, grid.spec))
    assert th.equal(grid(x, n_rows=th.tensor([2]))[2:], th.zeros(2, 8))
    other = FG.HashGrid(n_levels=4, features=2, log2_table_size=8, base_resolution=3, per_level_scale=1.5)
    assert not th.equal(other.table, grid.table)
    other.load_state_dict(grid.state_dict())
    assert th.equal(other.table, grid.table) and th.equal(other.lo, grid.lo) and th.equal(other(x), y)
    y.sum().backward()
    assert grid.table.grad is not None and float(grid.table.grad.abs().max()) > 0
    assert tuple(grid.double()(x.double()).shape) == (4, 8)
    for kw in (dict(lo=(0, 0)), dict(lo=(0, 0, 0), hi=(1, 0, 1))):
        with pytest.raises(ValueError, match="HashGrid: lo and hi"):
            FG.HashGrid(**kw)
    with pytest.raises(ValueError, match="hashgrid_spec: features"):
        FG.HashGrid(features=3)


# ---------------------------------------------------------------------------
# Library, binding and build lists
# ---------------------------------------------------------------------------
def _library():
    import capi_ctypes
    return RU.declare(capi_ctypes.load(), FUNCTIONS)


def test_the_c_layout_is_the_spec():
    lib = _library()
    specs = {(c.L, c.F, c.log2_T, c.R0, c.s) for c in _all_cases()} | {(16, 2, 19, 16, 1.38), (16, 1, 24, 2, 2.0), (13, 1, 24, 16, 2.0), (1, 8, 4, 1, 1.0)}
    assert len(specs) > 15
    for L, F, log2_T, R0, s in specs:
        spec = FG.hashgrid_spec(L, F, log2_T, R0, s)
        res = (C.c_int32 * L)(*spec.resolutions)
        out = (C.c_int64 * (L + 1))(*([-1] * (L + 1)))
        assert lib.dmr_hashgrid_layout(L, log2_T, res, out) == 0, lib.dmr_last_error()
        assert tuple(out) == spec.offsets, (L, F, log2_T, R0, s)
    assert any(sz == (r + 1) ** 3 for L, F, T, R0, s in specs for r, sz in zip(*FG.hashgrid_spec(L, F, T, R0, s)[:2]) if (r + 1) ** 3 < 1 << T)
    assert any(sz == 1 << T for L, F, T, R0, s in specs for sz in FG.hashgrid_spec(L, F, T, R0, s).sizes)


def test_library_exports_the_declared_symbols():
    RU.exports_declared(HEADER_TEXT, FUNCTIONS, absent=["dmr_hashgrid_stats"])   # (the ablation build's counters are not in the product)


def test_the_source_and_header_are_build_dependencies():
    RU.are_build_dependencies("dmr_hashgrid.hip", "dmesh_renderer_amd_hashgrid.h")


def test_binding_supports_it():
    from dmesh_renderer_amd import _C
    assert _C.SUPPORTS_FRAGMENT_HASHGRID is True
    assert callable(_C.hashgrid_rows) and callable(_C.hashgrid_rows_backward)
    for n in ("HashGridSpec", "hashgrid_spec", "hashgrid_rows", "hashgrid_rows_fused", "HashGrid"):
        assert n in FG.__all__ and callable(getattr(FG, n)) and n in FG.__doc__
    assert FG._FUSED["hashgrid_rows"] == ("SUPPORTS_FRAGMENT_HASHGRID", "row", "hash-grid encoding")
    assert _C.ABI_VERSION == 4 and _C.NUM_STAGES == 12   # (the header adds calls, not a version)


# ---------------------------------------------------------------------------
# Refusals of the functional layer, with CPU tensors: nothing reaches a device
# ---------------------------------------------------------------------------
def _inputs(N=6, dtype=th.float32):
    spec = FG.hashgrid_spec(3, 2, 6, 2, 2)
    return th.zeros(N, 3, dtype=dtype), th.zeros(spec.offsets[-1], 2, dtype=dtype), spec


def test_an_older_binding_says_rebuild(monkeypatch):
    class Old:
        SUPPORTS_FRAGMENT_MLP = True

    x, table, spec = _inputs()
    monkeypatch.setattr(dmr, "_C", Old())
    with pytest.raises(TypeError, match=r"hashgrid_rows_fused.*no fused row hash-grid encoding: rebuild.*" + TORCH_PATH):
        FG.hashgrid_rows_fused(x, table, spec)
    with pytest.raises(TypeError, match="rebuild"):   # ... before any other check
        FG.hashgrid_rows_fused(x[0], table, None)
    Old.SUPPORTS_FRAGMENT_HASHGRID = False
    with pytest.raises(TypeError, match="rebuild"):
        FG.hashgrid_rows_fused(x, table, spec)


def test_refusals_in_their_documented_order():
    """The arguments (ValueError, both paths: spec, x, table, n_rows), then the fused path's dtypes and devices (TypeError)."""
    x, table, spec = _inputs()
    for f, name in ((FG.hashgrid_rows, "hashgrid_rows"), (FG.hashgrid_rows_fused, "hashgrid_rows_fused")):
        with pytest.raises(ValueError, match=rf"{name}: spec must be a HashGridSpec"):
            f(x, table, (2, 4, 8))
        with pytest.raises(ValueError, match=rf"{name}: x must be \[N,3\], got \(6, 2\)"):
            f(x[:, :2], table, spec)
        with pytest.raises(ValueError, match=rf"{name}: x must be \[N,3\]"):
            f(x[0], table, spec)
        with pytest.raises(ValueError, match=rf"{name}: table must be \[offsets\[L\], F\] = \(155, 2\), got \(154, 2\)"):
            f(x, table[:-1], spec)
        with pytest.raises(ValueError, match=rf"{name}: table must be \[offsets\[L\], F\]"):
            f(x, th.zeros(155, 4), spec)
        with pytest.raises(ValueError, match=rf"{name}: n_rows must be None or a tensor of one element"):
            f(x, table, spec, n_rows=th.zeros(2, dtype=th.int32))
        with pytest.raises(ValueError, match=rf"{name}: n_rows must be None or a tensor of one element"):
            f(x, table, spec, n_rows=3)
        with pytest.raises(ValueError, match=rf"{name}: spec"):   # two at once: the first check wins
            f(x[0], table, None)
        with pytest.raises(ValueError, match=rf"{name}: x must be"):
            f(x[0], table[:-1], spec)
    xd, td, _ = _inputs(dtype=th.float64)
    with pytest.raises(ValueError, match="table must be"):   # a bad shape and a bad dtype: the shape is refused first
        FG.hashgrid_rows_fused(xd, td[:-1], spec)
    with pytest.raises(TypeError, match=r"hashgrid_rows_fused: x must be float32, got torch.float64; " + TORCH_PATH):
        FG.hashgrid_rows_fused(xd, table, spec)
    with pytest.raises(TypeError, match=r"hashgrid_rows_fused: table must be float32, got torch.float16; " + TORCH_PATH):
        FG.hashgrid_rows_fused(x, table.half(), spec)
    with pytest.raises(TypeError, match=r"hashgrid_rows_fused: n_rows must be int32, got torch.int64; " + TORCH_PATH):
        FG.hashgrid_rows_fused(x, table, spec, n_rows=th.zeros(1, dtype=th.int64))
    with pytest.raises(TypeError, match=r"hashgrid_rows_fused: x is on cpu: every tensor must be on one HIP device.*" + TORCH_PATH):
        FG.hashgrid_rows_fused(x, table, spec, n_rows=th.zeros(1, dtype=th.int32))
    res = list(spec.resolutions)
    for call in (lambda: dmr._C.hashgrid_rows(x, table, res, 6, None), lambda: dmr._C.hashgrid_rows_backward(x, table, res, 6, None, th.zeros(6, 6), True, True)):
        with pytest.raises(RuntimeError, match="no CPU path"):   # the binding below it refuses them too
            call()
    assert tuple(FG.HashGrid(3, 2, 6, 2, 2)(x).shape) == (6, 6)   # a CPU tensor takes the torch path


# ---------------------------------------------------------------------------
# Refusals of the C ABI, through ctypes with device pointers that are never dereferenced: every check runs before any HIP call.
# `resolutions` is a host array and is read.  No call here has wholly valid arguments and an output to write: none reaches a launch.
# ---------------------------------------------------------------------------
INTS = "N L F log2_T"
PTRS = {"dmr_hashgrid_rows": "resolutions x table n_rows y", "dmr_hashgrid_rows_backward": "resolutions x table n_rows grad_out dL_dx dL_dtable"}
SIZES = dict(N=1, L=3, F=2, log2_T=6)
RES = (C.c_int32 * 16)(2, 4, 8, *([1] * 13))
NULL_BY_DEFAULT = ("n_rows", "dL_dx", "dL_dtable")


def _res(*values):
    return (C.c_int32 * 16)(*values, *([1] * (16 - len(values))))


EVERY_CALL = {
    "N<0": (dict(N=-1), "bad rows"),
    "L=0": (dict(L=0), "L must be in 1..16, got 0"), "L=17": (dict(L=17), "L must be in 1..16, got 17"),
    "F=3": (dict(F=3), "F must be 1, 2, 4 or 8, got 3"), "F=16": (dict(F=16), "F must be 1, 2, 4 or 8, got 16"),
    "L*F=72": (dict(L=9, F=8), "L * F must be at most 64, got 72"),
    "log2_T=3": (dict(log2_T=3), "log2_T must be in 4..24, got 3"), "log2_T=25": (dict(log2_T=25), "log2_T must be in 4..24, got 25"),
    "null resolutions": (dict(resolutions=None), "null resolutions"),
    "R=0": (dict(resolutions=_res(2, 0, 8)), "resolutions[1] must be in 1..65536, got 0"),
    "R=65537": (dict(resolutions=_res(2, 4, 65537)), "resolutions[2] must be in 1..65536, got 65537"),
    "null x": (dict(x=None), "null x"), "null table": (dict(table=None), "null table"),
    # two at once: the first check wins
    "bad rows and bad L": (dict(N=-1, L=0), "bad rows"), "bad L and bad F": (dict(L=17, F=3), "L must be in 1..16, got 17"),
    "bad F and bad product": (dict(L=16, F=16), "F must be 1, 2, 4 or 8, got 16"), "bad product and bad log2_T": (dict(L=16, F=8, log2_T=2), "L * F must be at most 64, got 128"),
    "bad log2_T and null resolutions": (dict(log2_T=30, resolutions=None), "log2_T must be in 4..24, got 30"),
    "null resolutions and null x": (dict(resolutions=None, x=None), "null resolutions"),
    "bad resolution and null x": (dict(resolutions=_res(0, 4, 8), x=None), "resolutions[0] must be in 1..65536, got 0"),
    "null x and null table": (dict(x=None, table=None), "null x"),
}
PER_CALL = {
    "dmr_hashgrid_rows": {"null y": (dict(y=None), "null output"), "no rows, null x, null y": (dict(N=0, x=None, y=None), None),
                          "null table and null y": (dict(table=None, y=None), "null table")},
    "dmr_hashgrid_rows_backward": {"null grad_out": (dict(grad_out=None), "null grad_out"), "no gradient wanted": (dict(), None),
                                   "no rows, no gradient wanted": (dict(N=0, x=None, grad_out=None), None),
                                   "only dL_dx wanted, no rows": (dict(N=0, x=None, grad_out=None, dL_dx=D), None),
                                   "bad F although no gradient wanted": (dict(F=5), "F must be 1, 2, 4 or 8, got 5"),
                                   "null table and null grad_out": (dict(table=None, grad_out=None, dL_dx=D), "null table")},
}


def test_c_abi_refusals():
    lib = _library()
    RU.run_refusals(lib, INTS, PTRS, SIZES, NULL_BY_DEFAULT, EVERY_CALL, PER_CALL, special=dict(resolutions=RES))
    out = (C.c_int64 * 4)()
    for args, text in (((0, 6, RES, out), "L must be in 1..16, got 0"), ((3, 3, RES, out), "log2_T must be in 4..24, got 3"), ((3, 6, None, out), "null resolutions"),
                       ((3, 6, _res(2, 4, 0), out), "resolutions[2] must be in 1..65536, got 0"), ((3, 6, RES, None), "null output"), ((0, 3, None, None), "L must be in 1..16, got 0")):
        assert lib.dmr_hashgrid_layout(*args) == 1 and lib.dmr_last_error().decode() == "dmr_hashgrid_layout: " + text, args


# ---------------------------------------------------------------------------
# The case tables of the GPU tests
# ---------------------------------------------------------------------------
def test_dispatch_restated_as_the_unit_has_it():
    product = RU.dispatch_restated(HC, UNIT_TEXT, HEADER_TEXT, twice=HC.TWICE)
    assert tuple(FG.HASHGRID_FEATURES) == HC.FEATURES
    # the kernels the product launches are the ones every_instantiation lists: no <FF, false> forward
    assert "k_hashgrid_rows<FF, false>" not in product and "g_hg_stats" not in product and "p.dbg" not in product


def test_the_unit_waits_for_nothing_and_zeroes_nothing_by_memset():
    RU.waits_for_nothing([UNIT_TEXT], fill_calls=1)


def test_tables_reach_every_instantiation():
    full = HC.every_instantiation()
    assert len(full) == 4 + 12 + 1
    assert HC.instantiations(HC.TABLE) == {i for i in full if i[0] != "k_hashgrid_rows_backward" or i[1][1:] == (True, True)}
    assert HC.instantiations(_all_cases()) == full


def test_table_holds_the_shapes_that_can_go_wrong():
    t = HC.TABLE
    assert {0, 1, 63, 64, 65, 257} <= {c.N for c in t}
    assert sum(c.N > HC.MAX_GROUPS * HC.THREADS for c in t) == 2 and all(c.N < (HC.MAX_GROUPS + 2) * HC.THREADS for c in t)
    assert {1, 2, 8, 12, 16} <= {c.L for c in t} and {c.F for c in t} == set(HC.FEATURES)
    assert {1, 8, 32, 64} <= {c.L * c.F for c in t}
    assert all({f for c in t if c.L * c.F == w for f in (c.F,)} for w in (1, 8, 32, 64))
    assert {c.order for c in t} == {"ramp", "random", "same"}
    specs = [(c, _spec(c)) for c in t]
    dense = lambda c, s: [(r + 1) ** 3 <= 1 << c.log2_T for r in s.resolutions]
    assert any(c.log2_T == 4 and not any(dense(c, s)) for c, s in specs)                      # every level hashed
    assert any(all(dense(c, s)) and c.L > 1 for c, s in specs)                                 # every level dense
    for log2_T in (10, 14):                                                                    # the three grids, mixed levels
        for R0, sc, L in HC.GRIDS:
            mixed = [any(dense(c, s)) and not all(dense(c, s)) for c, s in specs if (c.log2_T, c.R0, c.s, c.L) == (log2_T, R0, sc, L)]
            assert mixed and (all(mixed) or (log2_T, R0) == (10, 16)), (log2_T, R0)   # (17^3 > 2^10: that grid is all hashed there)
    assert max(r for _, s in specs for r in s.resolutions) == 4096
    # 4096 * 2654435761 and 4097 * 805459861 exceed 2^32: the wrap runs on the device
    assert 4096 * 2654435761 >= 1 << 32 and 4097 * 805459861 >= 1 << 32


def test_the_boundary_band_is_small_on_every_case():
    """At most 3 % of a case's rows lie in the band the dL/dx comparison leaves out (the GPU test asserts it again)."""
    worst = 0.0
    for c in _all_cases():
        if c.N < 50:
            continue
        share = float(HC.boundary_band(HC.rows_of(c), _spec(c).resolutions).mean())
        worst = max(worst, share)
        assert share <= 0.03, (c, share)
    print(f"\nthe largest share of rows in the boundary band: {worst:.4f}")
    x = np.array([[0.5, 0.3, 0.3], [0.3, 0.3, 0.3], [0.3, 0.25 + 1e-7, 0.3], [0.3, 0.3, float("nan")]], dtype=np.float32)
    assert HC.boundary_band(x, (4,)).tolist() == [True, False, True, True]   # (NaN counts as 0: on a vertex)
