"""fragments.sh_rows / sh_rows_fused / packed_row_views / camera_origins / ViewSH without a GPU: the basis is orthonormal under
an exact quadrature and obeys the addition theorem (the two pin every constant), signs and channel order are the hand values at
four directions, gradcheck passes for x and origin at every degree, the gradient does not depend on a polynomial's form off the
sphere, the rules for the zero direction, for rows that are not read and for n_rows are what the docstring says, packed_row_views
is a Python loop's result, camera_origins is a hand-built look-at camera's eye, the library exports what
include/dmesh_renderer_amd_sh.h declares and the build lists hold the new files, the functional layer and the C ABI refuse what
the kernels do not take -- before anything reaches a device, in their documented order -- and the case tables of the GPU tests
(tests/sh_cases.py) reach every kernel instantiation the unit compiles."""
import math
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch as th

import row_units as RU
import sh_cases as SC
import dmesh_renderer_amd as dmr
from dmesh_renderer_amd import fragments as FG
from row_units import D

UNIT_TEXT, HEADER_TEXT = RU.unit_texts("dmr_sh.hip", "dmesh_renderer_amd_sh.h")
FUNCTIONS = ["dmr_packed_row_views", "dmr_sh_rows", "dmr_sh_rows_backward"]
TORCH_PATH = r"fragments\.sh_rows is the torch path"
NAMES = ("packed_row_views", "packed_row_views_fused", "sh_rows", "sh_rows_fused", "camera_origins", "ViewSH")


def _all_cases():
    return [c for rows in SC.tables().values() for c in rows]


def _unit_vectors(n, seed):
    d = th.randn(n, 3, dtype=th.float64, generator=th.Generator().manual_seed(seed))
    return d / d.norm(dim=1, keepdim=True)


# ---------------------------------------------------------------------------
# The basis
# ---------------------------------------------------------------------------
def test_orthonormal_under_an_exact_quadrature():
    """int Y_i Y_j over the sphere = delta_ij: Gauss-Legendre with 8 nodes in cos(theta) (exact to degree 15; the products have
    degree 6) times 16 equal steps in phi (exact for e^{i m phi} with |m| < 16; the products have |m| <= 6)."""
    ct, wt = np.polynomial.legendre.leggauss(8)
    phi = (np.arange(16) + 0.5) * (2 * math.pi / 16)
    c, p = np.meshgrid(ct, phi, indexing="ij")
    s = np.sqrt(1 - c * c)
    d = th.from_numpy(np.stack([s * np.cos(p), s * np.sin(p), c], -1).reshape(-1, 3))
    w = th.from_numpy((wt[:, None] * np.full((1, 16), 2 * math.pi / 16)).reshape(-1))
    Y = FG.sh_rows(d, 4)
    gram = (Y * w[:, None]).T @ Y
    err = float((gram - th.eye(16, dtype=th.float64)).abs().max())
    print(f"\nthe Gram matrix of the 16 channels against the identity: {err:.2e}")
    assert Y.dtype == th.float64 and tuple(Y.shape) == (128, 16) and err <= 1e-12
    for degree in (1, 2, 3):   # a lower degree is the first degree^2 channels
        assert th.equal(FG.sh_rows(d, degree), Y[:, :degree * degree])


def test_addition_theorem():
    """sum_m Y_lm(a) Y_lm(b) = (2l + 1) / (4 pi) P_l(a . b) on random pairs of directions, per band l = 0 .. 3."""
    a, b = _unit_vectors(200, 1), _unit_vectors(200, 2)
    Ya, Yb = FG.sh_rows(a, 4), FG.sh_rows(b, 4)
    t = (a * b).sum(1)
    legendre = [th.ones_like(t), t, (3 * t * t - 1) / 2, (5 * t ** 3 - 3 * t) / 2]
    for l in range(4):
        band = slice(l * l, (l + 1) * (l + 1))
        err = float(((Ya[:, band] * Yb[:, band]).sum(1) - (2 * l + 1) / (4 * math.pi) * legendre[l]).abs().max())
        print(f"\nthe addition theorem, l = {l}: {err:.2e}")
        assert err <= 1e-12


def test_signs_and_channel_order():
    """Hand values (Condon-Shortley signs; channel l l + l + m): at +z only m = 0 survives, with sqrt((2l+1) / (4 pi)); at +x and
    +y the values follow from the table's polynomials; (1,1,1)/sqrt(3) has xx = yy = zz = 1/3, xy = yz = xz = 1/3."""
    r = math.sqrt
    pi = math.pi
    want = {
        (0, 0, 1): {0: r(1 / (4 * pi)), 2: r(3 / (4 * pi)), 6: r(5 / (4 * pi)), 12: r(7 / (4 * pi))},
        (1, 0, 0): {0: r(1 / (4 * pi)), 3: -r(3 / (4 * pi)), 6: -0.5 * r(5 / (4 * pi)), 8: 0.5 * r(15 / (4 * pi)),
                    13: 0.4570457994644658, 15: -0.5900435899266435},
        (0, 1, 0): {0: r(1 / (4 * pi)), 1: -r(3 / (4 * pi)), 6: -0.5 * r(5 / (4 * pi)), 8: -0.5 * r(15 / (4 * pi)),
                    9: 0.5900435899266435, 11: 0.4570457994644658},
    }
    for d, values in want.items():
        y = FG.sh_rows(th.tensor([d], dtype=th.float64), 4)[0]
        for ch in range(16):
            assert abs(float(y[ch]) - values.get(ch, 0.0)) <= 1e-14, (d, ch, float(y[ch]))
    s = 1 / r(3)
    y = FG.sh_rows(th.tensor([[1.0, 1.0, 1.0]], dtype=th.float64), 4)[0]   # normalised by the call
    c1, c2, c3 = 0.4886025119029199, 1.0925484305920792, s ** 3
    hand = [0.28209479177387814, -c1 * s, c1 * s, -c1 * s, c2 / 3, -c2 / 3, 0.0, -c2 / 3, 0.0,
            -0.5900435899266435 * 2 * c3, 2.890611442640554 * c3, -0.4570457994644658 * 2 * c3, 0.3731763325901154 * -4 * c3,
            -0.4570457994644658 * 2 * c3, 0.0, -0.5900435899266435 * -2 * c3]
    assert float((y - th.tensor(hand, dtype=th.float64)).abs().max()) <= 1e-14
    # the header states the same table
    for number in ("0.28209479177387814", "0.4886025119029199", "1.0925484305920792", "0.31539156525252005", "0.5462742152960396",
                   "0.5900435899266435", "2.890611442640554", "0.4570457994644658", "0.3731763325901154", "1.445305721320277"):
        assert number in HEADER_TEXT and number in UNIT_TEXT, number


def _rows(n, B, seed, lo=0.5, hi=3.0):
    """x, origin, row_view in float64 with |x - origin[view]| in [lo, hi]"""
    g = th.Generator().manual_seed(seed)
    origin = th.rand(B, 3, dtype=th.float64, generator=g) * 4 - 2
    view = th.randint(0, B, (n,), generator=g).to(th.int32)
    length = lo + (hi - lo) * th.rand(n, 1, dtype=th.float64, generator=g)
    return origin[view.long()] + _unit_vectors(n, seed + 100) * length, origin, view


@pytest.mark.parametrize("degree", SC.DEGREES)
def test_gradcheck(degree):
    x, origin, view = _rows(9, 3, degree)
    x.requires_grad_(True)
    origin.requires_grad_(True)
    assert th.autograd.gradcheck(lambda a, o: FG.sh_rows(a, degree, origin=o, row_view=view), (x, origin), eps=1e-6, atol=1e-7)
    assert th.autograd.gradcheck(lambda a: FG.sh_rows(a, degree), (x,), eps=1e-6, atol=1e-7)
    assert th.autograd.gradcheck(lambda a, o: FG.sh_rows(a, degree, origin=o), (x, origin[:1]), eps=1e-6, atol=1e-7)
    n_rows = th.tensor([5])
    assert th.autograd.gradcheck(lambda a, o: FG.sh_rows(a, degree, origin=o, row_view=view, n_rows=n_rows), (x, origin), eps=1e-6, atol=1e-7)


def test_the_gradient_is_that_of_the_projected_derivative():
    """dL/dw = (gd - d (d . gd)) / n with gd the free-vector derivative of the table's polynomials -- what the kernels compute --
    against autograd through the model, and dL/dorigin = - the per-view sums."""
    x, origin, view = _rows(40, 3, 7)
    up = th.randn(40, 16, dtype=th.float64, generator=th.Generator().manual_seed(8))
    x.requires_grad_(True)
    origin.requires_grad_(True)
    gx, go = th.autograd.grad(FG.sh_rows(x, 4, origin=origin, row_view=view), [x, origin], grad_outputs=up)
    w = (x - origin[view.long()]).detach()
    n = w.norm(dim=1, keepdim=True)
    d = (w / n).requires_grad_(True)
    gd, = th.autograd.grad(FG._sh_polynomials(d, 4), [d], grad_outputs=up)
    dw = (gd - d * (d * gd).sum(1, keepdim=True)).detach() / n
    sums = th.zeros(3, 3, dtype=th.float64).index_add_(0, view.long(), -dw)
    assert float((gx - dw).abs().max()) <= 1e-12 and float((go - sums).abs().max()) <= 1e-12 and float(dw.abs().max()) > 0.1


def test_the_gradient_does_not_depend_on_the_form_off_the_sphere():
    """Channel 6 written as c (3 zz - 1) equals c (2 zz - xx - yy) on the sphere only; through d = w / |w| both give the same
    dL/dx: the projection removes what differs."""
    x, _, _ = _rows(30, 1, 9)
    c = 0.31539156525252005

    def grad_of(poly):
        a = x.clone().requires_grad_(True)
        d = a / a.norm(dim=1, keepdim=True)
        return th.autograd.grad(poly(d[:, 0], d[:, 1], d[:, 2]).sum(), [a])[0]

    homogeneous = grad_of(lambda X, Y, Z: c * (2 * Z * Z - X * X - Y * Y))
    on_sphere = grad_of(lambda X, Y, Z: c * (3 * Z * Z - 1))
    a = x.clone().requires_grad_(True)
    up = th.zeros(30, 16, dtype=th.float64)
    up[:, 6] = 1
    model, = th.autograd.grad(FG.sh_rows(a, 4), [a], grad_outputs=up)
    assert float((homogeneous - on_sphere).abs().max()) <= 1e-12 and float((model - on_sphere).abs().max()) <= 1e-12
    assert float(model.abs().max()) > 0.05


# ---------------------------------------------------------------------------
# The rules
# ---------------------------------------------------------------------------
ZERO_DIRECTION = [0.28209479177387814] + [0.0] * 15


@pytest.mark.parametrize("dtype", [th.float32, th.float64])
def test_zero_direction_rows(dtype):
    """The zero vector, NaN, Inf and |w| = 1e-9: d = (0, 0, 0) -- channel 0 alone --, dL/dx an exact 0, nothing to dL/dorigin;
    1e-7 is a direction like any other."""
    nan, inf = float("nan"), float("inf")
    origin = th.tensor([[0.5, -1.0, 2.0]], dtype=dtype, requires_grad=True)
    o = origin.detach()[0]
    rows = [o.tolist(), [nan, 0.0, 1.0], [inf, 0.0, 1.0], [-inf, inf, nan], (o + th.tensor([0.0, 1e-9, 0.0], dtype=dtype)).tolist(),
            (o + th.tensor([0.0, 0.0, 1.0], dtype=dtype)).tolist()]
    x = th.tensor(rows, dtype=dtype, requires_grad=True)
    y = FG.sh_rows(x, 4, origin=origin)
    up = th.randn(6, 16, dtype=dtype, generator=th.Generator().manual_seed(3))
    gx, go = th.autograd.grad(y, [x, origin], grad_outputs=up)
    assert bool(th.isfinite(y).all() and th.isfinite(gx).all() and th.isfinite(go).all())
    assert th.equal(y[:5].abs(), th.tensor([ZERO_DIRECTION] * 5, dtype=dtype)) and float(gx[:5].abs().max()) == 0.0
    assert float(gx[5].abs().max()) > 0 and th.equal(go[0], -gx[5])
    tiny = th.tensor([[0.0, 1e-7, 0.0], [0.0, 1e-9, 0.0]], dtype=dtype)
    yt = FG.sh_rows(tiny, 2)
    assert abs(float(yt[0, 1]) + 0.4886025119029199) < 1e-6 and float(yt[1, 1]) == 0.0
    if dtype == th.float32:   # |w|^2 overflows float32: not finite, the zero direction
        assert th.equal(FG.sh_rows(th.tensor([[1e30, 0.0, 0.0]]), 4)[0].abs(), th.tensor(ZERO_DIRECTION))


def test_rows_without_a_view_are_not_read():
    """row_view of -1 and of B (and beyond): exact zeros in y -- channel 0 too -- and in dL/dx, nothing added to dL/dorigin, and a
    NaN in such a row of x or of the upstream reaches nothing."""
    x, origin, view = _rows(12, 2, 11)
    view = view.clone()
    skip = th.tensor([1, 4, 5, 9])
    view[skip] = th.tensor([-1, 2, 7, -2 ** 31], dtype=th.int32)
    keep = th.ones(12, dtype=th.bool)
    keep[skip] = False
    up = th.randn(12, 9, dtype=th.float64, generator=th.Generator().manual_seed(12))
    xs = x.clone()
    xs[skip] = float("nan")
    xs.requires_grad_(True)
    origin.requires_grad_(True)
    y = FG.sh_rows(xs, 3, origin=origin, row_view=view)
    gx, go = th.autograd.grad(y, [xs, origin], grad_outputs=up)
    assert bool(th.isfinite(y).all() and th.isfinite(gx).all() and th.isfinite(go).all())
    assert float(y[skip].detach().abs().sum()) == 0.0 and float(gx[skip].abs().sum()) == 0.0
    xk, ok = x[keep].clone().requires_grad_(True), origin.detach().clone().requires_grad_(True)
    yk = FG.sh_rows(xk, 3, origin=ok, row_view=view[keep])
    gk, gok = th.autograd.grad(yk, [xk, ok], grad_outputs=up[keep])
    assert th.equal(y[keep], yk) and th.allclose(gx[keep], gk, rtol=0, atol=1e-14) and th.allclose(go, gok, rtol=0, atol=1e-13)


def test_n_rows_rule():
    x0, origin0, view = _rows(12, 2, 13)
    up = th.randn(12, 16, dtype=th.float64, generator=th.Generator().manual_seed(14))
    for n, dtype in ((0, th.int32), (5, th.int64), (12, th.int32), (40, th.int32), (-3, th.int32)):
        m = min(max(n, 0), 12)
        x = x0.clone()
        x[m:] = float("nan")
        u = up.clone()
        u[m:] = float("nan")
        x.requires_grad_(True)
        origin = origin0.clone().requires_grad_(True)
        y = FG.sh_rows(x, 4, origin=origin, row_view=view, n_rows=th.tensor([n], dtype=dtype))
        gx, go = th.autograd.grad(y, [x, origin], grad_outputs=th.nan_to_num(u))
        assert bool(th.isfinite(y).all() and th.isfinite(gx).all() and th.isfinite(go).all())
        assert float(y[m:].detach().abs().sum()) == 0.0 and float(gx[m:].abs().sum()) == 0.0
        if m:
            xs, os_ = x0[:m].clone().requires_grad_(True), origin0.clone().requires_grad_(True)
            ys = FG.sh_rows(xs, 4, origin=os_, row_view=view[:m])
            sx, so = th.autograd.grad(ys, [xs, os_], grad_outputs=up[:m])
            assert th.equal(y[:m].detach(), ys.detach()) and th.allclose(gx[:m], sx, rtol=0, atol=1e-14) and th.allclose(go, so, rtol=0, atol=1e-13)
        else:
            assert float(go.abs().sum()) == 0.0


def _lists(B, K, H, W, share, seed):
    g = th.Generator().manual_seed(seed)
    face = th.where(th.rand(B, K, H, W, generator=g) < share, th.randint(0, 50, (B, K, H, W), generator=g), th.full((B, K, H, W), -1)).to(th.int32)
    return SimpleNamespace(pix_to_face=face, bary=None, count=None)


def test_packed_row_views_against_a_loop():
    """Capacities below, at and above the count, and an exact pack: every row's view by a Python loop over the slots."""
    frag = _lists(3, 2, 5, 7, 0.5, 0)
    used = int(((frag.pix_to_face >= 0) & (frag.pix_to_face < 50)).sum())
    assert 20 < used < 3 * 2 * 5 * 7
    for capacity in (None, 0, used - 9, used, used + 6):
        packed = FG.pack_slots(frag, 50, capacity)
        want = [-1] * packed.rows
        for b in range(3):
            for k in range(2):
                for y in range(5):
                    for x in range(7):
                        r = int(packed.row[b, k, y, x])
                        if 0 <= r < packed.rows:
                            assert want[r] == -1
                            want[r] = b
        got = FG.packed_row_views(frag, packed)
        assert got.dtype == th.int32 and got.tolist() == want, capacity
        assert capacity is None or capacity <= used or set(want[used:]) == {-1}
        assert sorted(v for v in want if v >= 0) == [v for v in want if v >= 0]   # rows are numbered view-major
    with pytest.raises(ValueError, match=r"packed_row_views: packed.row must have frag.pix_to_face's shape"):
        FG.packed_row_views(frag, FG.pack_slots(_lists(3, 2, 5, 6, 0.5, 0), 50))


def _look_at(eye, target, up):
    """A row-major model-view matrix [4,4] (world -> camera, the camera looking down -z), written out by hand."""
    eye, target, up = (np.asarray(v, dtype=np.float64) for v in (eye, target, up))
    f = (target - eye) / np.linalg.norm(target - eye)
    s = np.cross(f, up)
    s /= np.linalg.norm(s)
    u = np.cross(s, f)
    m = np.eye(4)
    m[0, :3], m[1, :3], m[2, :3] = s, u, -f
    m[:3, 3] = -m[:3, :3] @ eye
    return m


def test_camera_origins_of_a_look_at_matrix():
    eyes = [(3.0, -2.0, 5.0), (0.0, 0.5, -4.0)]
    mv = th.from_numpy(np.stack([_look_at(e, (0.1, 0.2, 0.3), (0, 1, 0)) for e in eyes]))
    got = FG.camera_origins(mv)
    assert tuple(got.shape) == (2, 3) and float((got - th.tensor(eyes, dtype=th.float64)).abs().max()) <= 1e-12
    # the storage the kernels read: inv(mv.transpose(1, 2)) flattened holds the origin at [12..14] (pixel_ray, dmr_device.hpp)
    flat = th.inverse(mv.transpose(1, 2)).contiguous().reshape(2, 16)
    assert float((flat[:, 12:15] - got).abs().max()) <= 1e-12
    mv.requires_grad_(True)
    assert th.autograd.gradcheck(FG.camera_origins, (mv,), eps=1e-6, atol=1e-7)
    assert FG.camera_origins(mv.float()).dtype == th.float32
    for bad in (mv[0], mv[:, :3]):
        with pytest.raises(ValueError, match=r"camera_origins: mv_mats must be \[B,4,4\]"):
            FG.camera_origins(bad)


def test_module_on_cpu_rows():
    view = FG.ViewSH(3)
    assert view.out_features == 9 and view.degree == 3 and list(view.parameters()) == [] and FG.ViewSH().out_features == 16
    x, origin, rv = _rows(10, 2, 15)
    for xx, oo in ((x, origin), (x.float(), origin.float())):
        assert th.equal(view(xx, oo, rv), FG.sh_rows(xx, 3, origin=oo, row_view=rv))
        assert th.equal(view(xx, oo, rv, n_rows=th.tensor([4]))[4:], th.zeros(6, 9, dtype=xx.dtype))
    assert th.equal(view(x), FG.sh_rows(x, 3))
    x.requires_grad_(True)
    view(x, origin, rv).square().sum().backward()
    assert float(x.grad.abs().max()) > 0
    for bad in (0, 5, True, 2.0):
        with pytest.raises(ValueError, match="ViewSH: degree must be an int in 1..4"):
            FG.ViewSH(bad)


# ---------------------------------------------------------------------------
# Library, binding and build lists
# ---------------------------------------------------------------------------
def test_library_exports_the_declared_symbols():
    RU.exports_declared(HEADER_TEXT, FUNCTIONS)


def test_the_source_and_header_are_build_dependencies():
    RU.are_build_dependencies("dmr_sh.hip", "dmesh_renderer_amd_sh.h", extra=["dmr_deferred_common.hpp"])   # (RowPix, the packed unit's lanes)


def test_binding_supports_it():
    from dmesh_renderer_amd import _C
    assert _C.SUPPORTS_FRAGMENT_SH is True
    assert callable(_C.packed_row_views) and callable(_C.sh_rows) and callable(_C.sh_rows_backward)
    for n in NAMES:
        assert n in FG.__all__ and callable(getattr(FG, n)) and n in FG.__doc__
    assert FG._FUSED["sh_rows"] == ("SUPPORTS_FRAGMENT_SH", "row", "spherical-harmonics encoding")
    assert FG._FUSED["packed_row_views"] == ("SUPPORTS_FRAGMENT_SH", "packed row", "view map")
    assert (FG.SH_MAX_DEGREE, FG.SH_MAX_VIEWS) == (4, SC.MAX_VIEWS)
    assert _C.ABI_VERSION == 4 and _C.NUM_STAGES == 12   # (the header adds calls, not a version)
    # the module docstring's chain example, as the issue states it
    for line in ("view = FG.packed_row_views_fused(frag, packed)", "hit  = FG.interpolate_packed_fused(frag, packed, faces, verts)",
                 "enc  = th.cat([grid(hit, n_rows=n), FG.ViewSH(4)(hit, FG.camera_origins(mv_mats), view, n_rows=n)], 1)",
                 "image, T = FG.composite_values_packed_fused(frag, packed, faces_opacity, mlp(enc, n_rows=n))"):
        assert line in FG.__doc__, line


# ---------------------------------------------------------------------------
# Refusals of the functional layer, with CPU tensors: nothing reaches a device
# ---------------------------------------------------------------------------
def _inputs(N=6, B=2, dtype=th.float32):
    return th.ones(N, 3, dtype=dtype), th.zeros(B, 3, dtype=dtype), th.zeros(N, dtype=th.int32)


def test_an_older_binding_says_rebuild(monkeypatch):
    class Old:
        SUPPORTS_FRAGMENT_HASHGRID = True
        SUPPORTS_FRAGMENT_PACKED = True

    x, origin, view = _inputs()
    frag = _lists(1, 1, 2, 2, 0.5, 1)
    monkeypatch.setattr(dmr, "_C", Old())
    with pytest.raises(TypeError, match=r"sh_rows_fused.*no fused row spherical-harmonics encoding: rebuild.*" + TORCH_PATH):
        FG.sh_rows_fused(x, 4, origin=origin, row_view=view)
    with pytest.raises(TypeError, match="rebuild"):   # ... before any other check
        FG.sh_rows_fused(x[0], 9)
    with pytest.raises(TypeError, match=r"packed_row_views_fused.*no fused packed row view map: rebuild.*fragments\.packed_row_views is the torch path"):
        FG.packed_row_views_fused(frag, FG.pack_slots(frag, 50))
    Old.SUPPORTS_FRAGMENT_SH = False
    with pytest.raises(TypeError, match="rebuild"):
        FG.sh_rows_fused(x, 4)
    assert tuple(FG.ViewSH(2)(x).shape) == (6, 4)   # a CPU tensor takes the torch path: no binding needed


def test_refusals_in_their_documented_order():
    """The arguments (ValueError, both paths: x, degree, origin, row_view without origin, row_view's shape, several views without
    row_view, n_rows), then the fused path's dtypes and devices (TypeError)."""
    x, origin, view = _inputs()
    for f, name in ((FG.sh_rows, "sh_rows"), (FG.sh_rows_fused, "sh_rows_fused")):
        with pytest.raises(ValueError, match=rf"{name}: x must be \[N,3\], got \(6, 2\)"):
            f(x[:, :2], 4)
        with pytest.raises(ValueError, match=rf"{name}: x must be \[N,3\]"):
            f(x[0], 4)
        for bad in (0, 5, 2.0, True):
            with pytest.raises(ValueError, match=rf"{name}: degree must be an int in 1..4"):
                f(x, bad)
        with pytest.raises(ValueError, match=rf"{name}: origin must be \[B,3\], got \(2, 2\)"):
            f(x, 4, origin=origin[:, :2], row_view=view)
        with pytest.raises(ValueError, match=rf"{name}: origin must hold 1..1024 views, got 0"):
            f(x, 4, origin=origin[:0])
        with pytest.raises(ValueError, match=rf"{name}: origin must hold 1..1024 views, got 1025"):
            f(x, 4, origin=th.zeros(1025, 3), row_view=view)
        with pytest.raises(ValueError, match=rf"{name}: row_view needs origin"):
            f(x, 4, row_view=view)
        with pytest.raises(ValueError, match=rf"{name}: row_view must be \[N\] = \(6,\), got \(5,\)"):
            f(x, 4, origin=origin, row_view=view[:5])
        with pytest.raises(ValueError, match=rf"{name}: origin holds 2 views: row_view must tell"):
            f(x, 4, origin=origin)
        with pytest.raises(ValueError, match=rf"{name}: n_rows must be None or a tensor of one element"):
            f(x, 4, n_rows=th.zeros(2, dtype=th.int32))
        with pytest.raises(ValueError, match=rf"{name}: n_rows must be None or a tensor of one element"):
            f(x, 4, n_rows=3)
        with pytest.raises(ValueError, match=rf"{name}: x must be"):   # two at once: the first check wins
            f(x[0], 7)
        with pytest.raises(ValueError, match=rf"{name}: degree"):
            f(x, 7, origin=origin[:, :2])
        with pytest.raises(ValueError, match=rf"{name}: origin must be"):
            f(x, 4, origin=origin[:, :2], row_view=view[:5])
        with pytest.raises(ValueError, match=rf"{name}: row_view must be"):
            f(x, 4, origin=origin, row_view=view[:5], n_rows=3)
    xd, od, _ = _inputs(dtype=th.float64)
    with pytest.raises(ValueError, match="row_view must be"):   # a bad shape and a bad dtype: the shape is refused first
        FG.sh_rows_fused(xd, 4, origin=od, row_view=view[:5])
    with pytest.raises(TypeError, match=r"sh_rows_fused: x must be float32, got torch.float64; " + TORCH_PATH):
        FG.sh_rows_fused(xd, 4, origin=origin, row_view=view)
    with pytest.raises(TypeError, match=r"sh_rows_fused: origin must be float32, got torch.float16; " + TORCH_PATH):
        FG.sh_rows_fused(x, 4, origin=origin.half(), row_view=view)
    with pytest.raises(TypeError, match=r"sh_rows_fused: row_view must be int32, got torch.int64; " + TORCH_PATH):
        FG.sh_rows_fused(x, 4, origin=origin, row_view=view.long())
    with pytest.raises(TypeError, match=r"sh_rows_fused: n_rows must be int32, got torch.int64; " + TORCH_PATH):
        FG.sh_rows_fused(x, 4, origin=origin, row_view=view, n_rows=th.zeros(1, dtype=th.int64))
    with pytest.raises(TypeError, match=r"sh_rows_fused: x is on cpu: every tensor must be on one HIP device.*" + TORCH_PATH):
        FG.sh_rows_fused(x, 4, origin=origin, row_view=view, n_rows=th.zeros(1, dtype=th.int32))
    for call in (lambda: dmr._C.sh_rows(x, 4, origin, view, None), lambda: dmr._C.sh_rows_backward(x, 4, origin, view, None, th.zeros(6, 16), True, True),
                 lambda: dmr._C.packed_row_views(th.zeros(1, 1, 2, 2, dtype=th.int32), 3)):
        with pytest.raises(RuntimeError, match="no CPU path"):   # the binding below it refuses them too
            call()
    # packed_row_views_fused: the lists, the pack, then dtypes and devices
    frag = _lists(2, 2, 3, 4, 0.5, 2)
    packed = FG.pack_slots(frag, 50)
    with pytest.raises(ValueError, match=r"packed_row_views_fused: frag.pix_to_face must be \[B,K,H,W\]"):
        FG.packed_row_views_fused(SimpleNamespace(pix_to_face=frag.pix_to_face[0], bary=None), packed)
    with pytest.raises(ValueError, match=r"packed_row_views_fused: packed.row must have frag.pix_to_face's shape"):
        FG.packed_row_views_fused(frag, packed._replace(row=packed.row[:1]))
    with pytest.raises(ValueError, match=r"packed_row_views_fused: packed.rows must be a non-negative int"):
        FG.packed_row_views_fused(frag, packed._replace(rows=-1))
    with pytest.raises(TypeError, match=r"packed_row_views_fused: packed.row must be int32, got torch.int64; fragments\.packed_row_views is the torch path"):
        FG.packed_row_views_fused(frag, packed._replace(row=packed.row.long()))
    with pytest.raises(TypeError, match=r"packed_row_views_fused: frag.pix_to_face is on cpu.*fragments\.packed_row_views is the torch path"):
        FG.packed_row_views_fused(frag, packed)


# ---------------------------------------------------------------------------
# Refusals of the C ABI, through ctypes with device pointers that are never dereferenced: every check runs before any HIP call.
# No call here has wholly valid arguments and an output to write: none reaches a launch.
# ---------------------------------------------------------------------------
INTS = "N degree B"
PTRS = {"dmr_sh_rows": "x origin row_view n_rows y", "dmr_sh_rows_backward": "x origin row_view n_rows grad_out dL_dx dL_dorigin"}
SIZES = dict(N=1, degree=4, B=2)
NULL_BY_DEFAULT = ("n_rows", "dL_dx", "dL_dorigin")
EVERY_CALL = {
    "N<0": (dict(N=-1), "bad rows"),
    "degree=0": (dict(degree=0), "degree must be in 1..4, got 0"), "degree=5": (dict(degree=5), "degree must be in 1..4, got 5"),
    "row_view without origin": (dict(origin=None), "row_view without origin"),
    "B=0": (dict(B=0), "B must be in 1..1024, got 0"), "B=1025": (dict(B=1025), "B must be in 1..1024, got 1025"),
    "null x": (dict(x=None), "null x"),
    # two at once: the first check wins
    "bad rows and bad degree": (dict(N=-1, degree=9), "bad rows"), "bad degree and no origin": (dict(degree=-1, origin=None), "degree must be in 1..4, got -1"),
    "no origin and bad B": (dict(origin=None, B=0), "row_view without origin"), "bad B and null x": (dict(B=-3, x=None), "B must be in 1..1024, got -3"),
}
PER_CALL = {
    "dmr_sh_rows": {"null y": (dict(y=None), "null output"), "no rows, null x, null y": (dict(N=0, x=None, y=None), None),
                    "null x and null y": (dict(x=None, y=None), "null x"),
                    "directions: B is not read": (dict(N=0, origin=None, row_view=None, B=-5), None)},
    "dmr_sh_rows_backward": {"null grad_out": (dict(grad_out=None), "null grad_out"), "no gradient wanted": (dict(), None),
                             "no rows, no gradient wanted": (dict(N=0, x=None, grad_out=None), None),
                             "only dL_dx wanted, no rows": (dict(N=0, x=None, grad_out=None, dL_dx=D), None),
                             "bad degree although no gradient wanted": (dict(degree=7), "degree must be in 1..4, got 7"),
                             "dL_dorigin without origin": (dict(origin=None, row_view=None, dL_dorigin=D), "dL_dorigin without origin"),
                             "null grad_out and dL_dorigin without origin": (dict(origin=None, row_view=None, grad_out=None, dL_dorigin=D), "null grad_out"),
                             "null x and null grad_out": (dict(x=None, grad_out=None, dL_dx=D), "null x")},
}
VIEWS_CALL = [  # (B, K, H, W, N, row, view_out) -> text (None: returns 0 without a launch)
    ((-1, 1, 2, 2, 3, D, D), "bad dimensions"), ((1, 1, 2, -2, 3, D, D), "bad dimensions"), ((1, 1, 2, 2, -3, D, D), "bad dimensions"),
    ((1, 0, 2, 2, 3, D, D), "K must be in 1..32, got 0"), ((1, 33, 2, 2, 3, D, D), "K must be in 1..32, got 33"),
    ((2, 32, 8192, 8192, 3, D, D), "problem too large"), ((1, 1, 2, 2, 3, None, D), "null row"), ((1, 1, 2, 2, 3, D, None), "null output"),
    ((-1, 0, 2, 2, 3, None, None), "bad dimensions"), ((1, 0, 1 << 20, 1 << 20, 3, None, None), "K must be in 1..32, got 0"),
    ((2, 32, 8192, 8192, 3, None, None), "problem too large"), ((1, 1, 2, 2, 3, None, None), "null row"),
    ((1, 1, 2, 2, 0, D, None), None), ((0, 1, 2, 2, 3, None, D), None), ((1, 1, 0, 2, 3, None, D), None), ((1, 4, 2, 0, 0, None, None), None),
]


def test_c_abi_refusals():
    import capi_ctypes
    lib = RU.declare(capi_ctypes.load(), FUNCTIONS)
    RU.run_refusals(lib, INTS, PTRS, SIZES, NULL_BY_DEFAULT, EVERY_CALL, PER_CALL)
    for args, text in VIEWS_CALL:
        ret = lib.dmr_packed_row_views(*args, None)
        got = lib.dmr_last_error().decode() if ret else ""
        assert (ret, got) == ((0, "") if text is None else (1, "dmr_packed_row_views: " + text)), (args, got)
    # the order the header documents is the order tested above
    order = re.sub(r"\s*\n \* ", " ", HEADER_TEXT[HEADER_TEXT.index("The order, for the two encoding calls"):])
    at = [order.index(w) for w in ('"bad rows"', "degree,", "row_view without origin", "B (when origin", "null x", "a null output (dmr_sh_rows,", "null grad_out",
                                   "dL_dorigin without origin", '"bad dimensions"', "K outside", '"problem too large"', "null row", "null output (when N > 0)")]
    assert at == sorted(at)


# ---------------------------------------------------------------------------
# The case tables of the GPU tests
# ---------------------------------------------------------------------------
def test_dispatch_restated_as_the_unit_has_it():
    product = RU.dispatch_restated(SC, UNIT_TEXT, HEADER_TEXT, twice=SC.TWICE)
    assert all(SC.via_lds(d) == (d >= 3) and not SC.loads_via_lds(d) for d in SC.DEGREES) and SC.DEGREES == tuple(range(1, FG.SH_MAX_DEGREE + 1))
    # the kernels the product launches are the ones every_instantiation lists: no <D, !L> shape
    assert "!L>" not in product and "ablate_bits" not in product and "!L>" in UNIT_TEXT


def test_the_unit_waits_for_nothing_and_zeroes_nothing_by_memset():
    RU.waits_for_nothing([UNIT_TEXT], fill_calls=2, extra_forbidden=["zero_on("])   # (dL_dorigin and view_out; nothing by the shading units' zero_on)


def test_tables_reach_every_instantiation():
    full = SC.every_instantiation()
    assert len(full) == 4 + 12 + 2
    rows_only = {i for i in full if i[0] != "k_sh_row_views"}
    assert SC.instantiations(_all_cases()) == rows_only          # (k_sh_row_views: the VIEW_SHAPES and the chains)
    pairs = {i for i in rows_only if i[0] != "k_sh_rows_backward" or i[1][1:3] == (True, True)}
    assert SC.instantiations(SC.TABLE) == pairs | {("k_sh_rows_backward", (d, True, False, SC.loads_via_lds(d))) for d in (2, 3, 4)}   # (origin=None)


def test_table_holds_the_shapes_that_can_go_wrong():
    t = SC.TABLE
    assert {0, 1, 63, 64, 65, 255, 256, 257} <= {c.N for c in t}
    assert sum(c.N > SC.MAX_GROUPS * SC.THREADS for c in t) == 2 and all(c.N < (SC.MAX_GROUPS + 2) * SC.THREADS for c in t)
    for shape in (False, True):   # every degree of each store shape, below and above a workgroup's tile
        for d in (d for d in SC.DEGREES if SC.via_lds(d) == shape):
            assert any(c.degree == d and c.N <= SC.THREADS for c in t) and any(c.degree == d and c.N > 2 * SC.THREADS for c in t), d
    assert {c.B for c in t} == {1, 2, 5} and {c.layout for c in t} == set(SC.LAYOUTS) and {c.form for c in t} == {"views", "single", "dirs"}
    for c in t:
        v = SC.views_of(c)
        x, origin = SC.rows_of(c)
        assert v.shape == (c.N,) and x.shape == (c.N, 3) and origin.shape == (c.B, 3) and x.dtype == np.float32
        waves = v[:c.N - c.N % 64].reshape(-1, 64)
        mixed = (waves != waves[:, :1]).any(1)
        if c.layout in ("one", "wave", "group"):
            assert not mixed.any()                    # every wave of one view: the wave's sum
        if c.layout in ("mixed", "shuffled") and c.N >= 64 and c.B > 1:
            assert mixed.all()                        # every wave of several views: the per-lane adds
        if c.layout == "wave" and c.N > 64:
            assert (waves[1:, 0] != waves[:-1, 0]).all()
        if c.layout == "group" and c.N > 2 * SC.THREADS:
            tiles = v[:c.N - c.N % SC.THREADS].reshape(-1, SC.THREADS)
            assert not (tiles != tiles[:, :1]).any() and (tiles[1:, 0] != tiles[:-1, 0]).all()
        if c.layout == "holes" and c.N > 100:
            assert (v == -1).any() and (v >= c.B).any() and ((v >= 0) & (v < c.B)).sum() > c.N // 2
        if c.form == "views" and c.N:   # |w| in [0.5, 3] on the rows that are read
            ok = (v >= 0) & (v < c.B)
            n = np.linalg.norm(x[ok].astype(np.float64) - origin[v[ok]], axis=1)
            assert n.size == 0 or (n.min() > 0.49 and n.max() < 3.01)
    assert {c.degree for c in SC.MISALIGNED} == set(SC.DEGREES)
    assert (1, 1, 1, 1, 1.0) in SC.VIEW_SHAPES and (2, 5, 17, 33, 0.4) in SC.VIEW_SHAPES and {s[1] for s in SC.VIEW_SHAPES} == {1, 5, 32}
    assert any(s[0] * ((s[3] + 63) // 64) * ((s[2] + 3) // 4) == 258 for s in SC.VIEW_SHAPES)   # 258 workgroups' worth
    assert any(s[4] == 0.0 for s in SC.VIEW_SHAPES) and any(s[4] == 1.0 for s in SC.VIEW_SHAPES)
