"""fragments.envmap_pyramid_fused, envmap_lod_rows_fused and EnvMapPyramid on the GPU (csrc/dmr_envmap_lod.hip: k_envmap_pyramid_base,
k_envmap_pyramid_level, k_envmap_pyramid_backward, k_envmap_lod_rows, k_envmap_lod_rows_backward; csrc/dmr_rows_common.hip:
k_rows_fill).  The builder against fragments.envmap_pyramid in float32 on the CPU, bit for bit, both directions.  The lookup against
fragments.envmap_lod_rows evaluated in float64 on the CPU, on the same float32 inputs cast up: the case table of
tests/envmap_lod_cases.py (every instantiation; N around a wave, a workgroup's tile and the capped grid; C = 1 .. 16; pyramids from
1 x 1 L1 to 64 x 128 L7; envmap_cases' six layouts; lod uniform over both clamps, all one value, exact integers, all in one pair),
special lod and d between sentinels, a strided lod, buffers off a 16-byte boundary, n_rows on the device, the seven subsets of
the gradients, the existing unit at lod <= 0, a replayed HIP graph, and the chain of the module docstring.

Inputs: |d| in [0.5, 3], base map and upstream ~ N(0,1); the lookup's pyramid is fragments.envmap_pyramid of the base map in float32
on the CPU.  lod reaches every model as the same float32 values, so the level choice never differs.  Errors are max |got - ref| /
max |ref| (row_units.rel_to_largest).  Bounds (the project's own): y within max(FWD_TOL = 1e-5, 4 x the yardstick), gradients within
max(GRAD_TOL = 1e-4, 4 x the yardstick), the yardstick being fragments.envmap_lod_rows in float32 on the CPU against float64 on the
same case; never anything the kernels gave.  For the dL_dd comparison only, rows within 1e-3 texel of a cell line of either level
they use, or with rho2 < 1e-4, carry no upstream (envmap_lod_cases.no_dd_upstream; at most max(5 rows, 3 %) of a case's rows,
asserted here and, from the float64 model alone, in tests/test_envmap_lod_cpu.py): there float32 and float64 may sit in different
cells and the derivative, which holds the cell constant, jumps.  y, dL_dlod and dL_dpyramid are continuous there and get no
exclusion.  Every case prints what it measured (pytest -s).

MEASURED on the MI355X, the largest figure over the table's 25 cases (in brackets float32 torch on the CPU on the same cases, the
yardstick): y 8.7e-6 (9.5e-6), dL_dd 6.2e-6 (6.6e-6), dL_dlod 9.2e-6 (1.1e-5), dL_dpyramid 9.6e-7 (3.1e-6); at most 4 of 255 rows
(1.6 %) of a case without upstream in the dL_dd comparison; every case runs the backward's full instantiation and the one without dL_dd.  The builder: both directions equal the float32 model on all 8 shapes,
aligned and one float off.  The 4 misaligned calls and the strided lod (a column of [N,4], an [N,1] view, stride 7 through the C ABI)
give the aligned, contiguous calls' y, dL_dd and dL_dlod bit for bit, dL_dpyramid too.  Special rows: y 1.1e-6, dL_dd 1.4e-6, dL_dlod
8.4e-7, dL_dpyramid 6.9e-7, exact zeros where the model has them, every sentinel word unchanged.  Each of the seven want-combinations:
dL_dd and dL_dlod equal to the full call's, dL_dpyramid equal too.  At lod <= 0 and at L == 1: y and dL_dd differ from
envmap_rows_fused on level 0 by exactly 0.  Graph replays against eager (n_rows 500 -> 90 -> 700 of 700 rows): the pyramid, y, dL_dd
and dL_dlod equal, dL_dpyramid within 2.7e-8 and 1.2e-6 from float64, dL_denvmap within 4.3e-8 and 1.7e-6, exact zeros in the 40,
313 and 258 pyramid texels out of every row's reach (envmap_lod_cases.may_touch).  The chain: image 1.5e-7, verts.grad 1.5e-7,
envmap.grad 4.1e-7, the MLP's gradients to 1.1e-7.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch as th

import envmap_lod_cases as LC
import dmesh_renderer_amd as dmr
from dmesh_renderer_amd import fragments as FG
from dmesh_renderer_amd import scenes
from harness import TRI_ARGS, capture_replay, replay
from row_units import FWD_TOL, GRAD_TOL, check, counts_calls, guarded, intact, models, n_rows_counts, within_floors
from row_units import rel_to_largest as _rel
from util import rel_err, sum_order_tol

pytestmark = pytest.mark.gpu
GRADS = {"d": 0, "l": 1, "p": 2}   # a want's letters -> the position among (d, lod, pyramid)


def _spec(c):
    return (c.He, c.We, c.L)


@functools.lru_cache(maxsize=None)
def _inputs(c):
    """float32 CPU tensors of a case: d, lod, the pyramid (the float32 CPU model's, of the case's base map), the upstream, and the
    upstream of the dL_dd comparison."""
    d, lod = LC.directions_of(c), LC.lod_of(c)
    pyr = FG.envmap_pyramid(th.from_numpy(LC.pyramid_base_of(c)), c.L)
    g = th.Generator().manual_seed(1000 * c.seed + 7 * c.N + 13 * c.C + c.He)
    up = th.randn(c.N, c.C, generator=g)
    quiet = th.from_numpy(LC.no_dd_upstream(d, lod, c.He, c.We, c.L))
    return dict(d=th.from_numpy(d), lod=th.from_numpy(lod), pyr=pyr, up=up, up_d=th.where(quiet.unsqueeze(1), th.zeros(()), up), quiet=quiet)


def _run(f, c, t, device, dtype, n=None, want=None):
    """{"y", "d" (dL/dd, from the upstream without the rows near a cell line), "l" (dL/dlod) and "p" (dL/dpyramid), both from the full
    upstream} of one forward and the backward calls of envmap_lod_cases.backward_calls -- one for everything wanted, of which dL/dd
    is kept (a "dlp" case runs the full instantiation, the BIG case with it), and one for dL/dlod and dL/dpyramid without dL/dd --,
    as numpy; n: the n_rows count or None; want: c.want unless given."""
    want = want or c.want
    x = [t[k].clone().to(device, dtype).requires_grad_(w in want) for k, w in (("d", "d"), ("lod", "l"), ("pyr", "p"))]
    nr = None if n is None else th.tensor([n], dtype=th.int32, device=device)
    y = f(x[0], x[1], x[2], _spec(c), n_rows=nr)
    out = {"y": y.detach().cpu().numpy()}
    if "d" in want:
        out["d"] = th.autograd.grad(y, [x[GRADS[w]] for w in want], grad_outputs=t["up_d"].to(device, dtype), retain_graph=True)[want.index("d")].cpu().numpy()
    rest = [w for w in want if w != "d"]
    if rest:
        grads = th.autograd.grad(y, [x[GRADS[w]] for w in rest], grad_outputs=t["up"].to(device, dtype))
        out.update({w: g.cpu().numpy() for w, g in zip(rest, grads)})
    return out


@functools.lru_cache(maxsize=None)
def _models(c, n=None):
    """fragments.envmap_lod_rows on the CPU in float64 and in float32 -> (reference, {name: (the bound of the case, the yardstick)})."""
    return models(_run, FG.envmap_lod_rows, c._replace(want="dlp"), _inputs(c), n, _rel)


def _check(what, c, got, n=None):
    return check(what, *_models(c, n), got, _rel)


@pytest.mark.parametrize("i", range(len(LC.TABLE)))
def test_table(hip_device, i):
    c = LC.TABLE[i]
    t = _inputs(c)
    out = int(t["quiet"].sum())
    print(f"\n{c}: {out} of {c.N} rows carry no upstream in the dL_dd comparison (cap {LC.exclusion_cap(c.N)})")
    assert out <= LC.exclusion_cap(c.N)
    got = _run(FG.envmap_lod_rows_fused, c, t, hip_device, th.float32)
    ref = _check(str(c), c, got)
    if c.N == 0:
        assert ref["y"].shape == (0, c.C) and float(np.abs(got["p"]).max()) == 0.0 and got["l"].shape == (0,)
        return
    assert float(np.abs(ref["y"]).max()) > 0 and float(np.abs(ref["p"]).max()) > 0
    p = LC.places64(t["d"].numpy(), t["lod"].numpy(), c.He, c.We, c.L)
    assert not (got["l"][~p["inside"]] != 0).any() and not (ref["l"][~p["inside"]] != 0).any()   # an exact 0 wherever lod is not inside (0, L-1)
    assert (c.L == 1 or c.N < 63) or float(np.abs(ref["l"]).max()) > 0
    # no row adds into a level it does not use, or away from its cell: exact zeros there (always checked: may_touch is a superset)
    touched = LC.may_touch(t["d"].numpy(), t["lod"].numpy(), c.He, c.We, c.L)
    for k in range(2):
        assert touched[p["rows"][k][:, p["w"][k] != 0].ravel()].all()
    print(f"\n{int((~touched).sum())} of {touched.size} pyramid texels out of every row's reach: exact zeros")
    assert float(np.abs(got["p"][~touched]).sum()) == 0.0 and float(np.abs(ref["p"][~touched]).sum()) == 0.0
    # the sum identity: the eight weights of a row sum to 1.  Float32 sums of the upstream's terms: within 1e-5 of the sum of their magnitudes
    total, want = got["p"].astype(np.float64).sum(0), t["up"].double().sum(0).numpy()
    assert np.abs(total - want).max() <= 1e-5 * max(1.0, float(t["up"].abs().sum(0).max())), (total, want)


# ---------------------------------------------------------------------------
# The builder: bit for bit the float32 model
# ---------------------------------------------------------------------------
def _c_calls():
    from dmesh_renderer_amd import _C
    return LC.declare(C.CDLL(_C.library_path()))


@pytest.mark.parametrize("i", range(len(LC.BUILDER)))
def test_builder_equals_the_float32_model_bit_for_bit(hip_device, i):
    """Forward and backward, through the Function and, one float off a 16-byte boundary between sentinels, through the C ABI."""
    Cn, He, We, L = LC.BUILDER[i]
    dev, g = hip_device, th.Generator().manual_seed(100 + i)
    env = th.randn(He, We, Cn, generator=g).requires_grad_(True)
    pyr = FG.envmap_pyramid(env, L)
    up = th.randn(pyr.shape, generator=g)
    want_de, = th.autograd.grad(pyr, [env], grad_outputs=up)
    e = env.detach().to(dev).requires_grad_(True)
    got = FG.envmap_pyramid_fused(e, L)
    got_de, = th.autograd.grad(got, [e], grad_outputs=up.to(dev))
    f_eq, b_eq = th.equal(got.detach().cpu(), pyr.detach()), th.equal(got_de.cpu(), want_de)
    print(f"\nbuilder C {Cn}, {He} x {We}, L {L} (T = {pyr.shape[0]}): forward equal {f_eq}, backward equal {b_eq}")
    assert tuple(got.shape) == tuple(pyr.shape) and f_eq and b_eq
    assert not FG.envmap_pyramid_fused(e.detach(), L).requires_grad
    lib, stream = _c_calls(), th.cuda.current_stream(dev).cuda_stream
    T = pyr.shape[0]
    sizes = dict(env=He * We * Cn, pyr=T * Cn, up=T * Cn, de=He * We * Cn)
    bufs = {k: guarded(dev, n, 1) for k, n in sizes.items()}
    bufs["env"][1].copy_(env.detach().to(dev).flatten())
    bufs["up"][1].copy_(up.to(dev).flatten())
    p = {k: b[1].data_ptr() for k, b in bufs.items()}
    with th.cuda.device(dev):
        assert lib.dmr_envmap_pyramid(Cn, He, We, L, p["env"], p["pyr"], stream) == 0, lib.dmr_last_error()
        assert lib.dmr_envmap_pyramid_backward(Cn, He, We, L, p["up"], p["de"], stream) == 0, lib.dmr_last_error()
    th.cuda.synchronize()
    assert all(intact(bufs[k][0], n, 1) for k, n in sizes.items())
    assert th.equal(bufs["pyr"][1].cpu().view(T, Cn), pyr.detach()) and th.equal(bufs["de"][1].cpu().view(He, We, Cn), want_de)


# ---------------------------------------------------------------------------
# The lookup through the C ABI: sentinels, a strided lod, and buffers one float off a 16-byte boundary
# ---------------------------------------------------------------------------
def _call_pair(lib, dev, N, Cn, spec, d, lod, pyr, up, off=0, stride=1, n_rows=None):
    """One forward and one backward through the C ABI with every tensor inside a guarded buffer `off` floats off alignment, lod
    `stride` floats apart -> (y [N,C], dL_dd [N,3], dL_dlod [N], dL_dpyramid [T,C]) as numpy; asserts that every sentinel is unchanged."""
    He, We, L = spec
    T = pyr.shape[0]
    stream = th.cuda.current_stream(dev).cuda_stream
    sizes = dict(d=N * 3, lod=max((N - 1) * stride + 1, 1), pyr=T * Cn, y=N * Cn, up=N * Cn, dd=N * 3, dl=N, dp=T * Cn)
    bufs = {k: guarded(dev, n, off) for k, n in sizes.items()}
    bufs["d"][1].copy_(d.to(dev).flatten())
    bufs["lod"][1].fill_(float("nan"))          # (what lies between the rows' lod is not read)
    bufs["lod"][1][::stride][:N].copy_(lod.to(dev))
    bufs["pyr"][1].copy_(pyr.to(dev).flatten())
    bufs["up"][1].copy_(up.to(dev).flatten())
    p = {k: b[1].data_ptr() for k, b in bufs.items()}
    nr = None if n_rows is None else n_rows.data_ptr()
    with th.cuda.device(dev):
        assert lib.dmr_envmap_lod_rows(N, Cn, He, We, L, stride, p["d"], p["lod"], p["pyr"], nr, p["y"], stream) == 0, lib.dmr_last_error()
        assert lib.dmr_envmap_lod_rows_backward(N, Cn, He, We, L, stride, p["d"], p["lod"], p["pyr"], nr, p["up"], p["dd"], p["dl"], p["dp"], stream) == 0, lib.dmr_last_error()
    th.cuda.synchronize()
    for k, n in sizes.items():
        assert intact(bufs[k][0], n, off), k
    return (bufs["y"][1].cpu().numpy().reshape(N, Cn), bufs["dd"][1].cpu().numpy().reshape(N, 3), bufs["dl"][1].cpu().numpy(), bufs["dp"][1].cpu().numpy().reshape(T, Cn))


@pytest.mark.parametrize("i", range(len(LC.MISALIGNED)))
def test_one_float_off_a_16_byte_boundary(hip_device, i):
    """The same call with every buffer at base + 4 bytes (no float4 reads): y, dL_dd and dL_dlod bit-equal to the aligned call's,
    dL_dpyramid within the suite's summation-order tolerance; the words around every buffer unchanged."""
    c, dev = LC.MISALIGNED[i], hip_device
    t, lib = _inputs(c), _c_calls()
    a, b = (_call_pair(lib, dev, c.N, c.C, _spec(c), t["d"], t["lod"], t["pyr"], t["up_d"], off) for off in (0, 1))
    e_p = _rel(b[3], a[3])
    print(f"\n{c}: y equal {np.array_equal(a[0], b[0])}, dL_dd equal {np.array_equal(a[1], b[1])}, dL_dlod equal {np.array_equal(a[2], b[2])}, dL_dpyramid {e_p:.2e} from the aligned call")
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and e_p <= sum_order_tol("pyramid")
    ref, bounds = _models(c)
    assert _rel(b[0], ref["y"]) <= bounds["y"][0] and _rel(b[1], ref["d"]) <= bounds["d"][0]


@pytest.mark.parametrize("i", range(len(LC.STRIDED)))
def test_strided_lod(hip_device, i):
    """lod read as a column of an [N,4] tensor, in place (the binding makes no copy: the column's NaN neighbours would otherwise not
    matter, so the C ABI is given them too): y and all gradients bit-equal to the contiguous call."""
    c, dev = LC.STRIDED[i], hip_device
    t = _inputs(c)
    wide = th.full((c.N, 4), float("nan"))
    wide[:, 3] = t["lod"]
    outs = []
    for lod in (t["lod"].to(dev), wide.to(dev)[:, 3], wide.to(dev)[:, 3:4]):
        x = [t["d"].to(dev).requires_grad_(True), lod.requires_grad_(True), t["pyr"].to(dev).requires_grad_(True)]
        y = FG.envmap_lod_rows_fused(x[0], x[1], x[2], _spec(c))
        grads = th.autograd.grad(y, x, grad_outputs=t["up_d"].to(dev))
        assert grads[1].shape == lod.shape and grads[1].is_contiguous()
        outs.append([y.detach().cpu().numpy()] + [g.cpu().numpy().reshape(-1) for g in grads])
    assert not wide.to(dev)[:, 3].is_contiguous()
    for other in outs[1:]:
        same = [np.array_equal(a, b) for a, b in zip(outs[0], other)]
        print(f"\n{c}: a strided lod against the contiguous call: y, dL_dd, dL_dlod, dL_dpyramid equal {same}")
        assert all(same)
    lib = _c_calls()
    a, b = (_call_pair(lib, dev, c.N, c.C, _spec(c), t["d"], t["lod"], t["pyr"], t["up_d"], 0, stride) for stride in (1, 7))
    assert all(np.array_equal(x, z) for x, z in zip(a, b))
    _check(str(c) + " strided", c, dict(y=b[0], d=b[1]))


def test_special_lod_and_special_rows(hip_device):
    """Special lod (NaN, +-Inf, -0.0, 1e30, L-1 exactly, just below it) on ordinary rows and special d (zero, NaN, +-Inf, 1e30, a
    denormal, the exact poles, the exact seam) with NaN lod, in every wave of three, every tensor between sentinels: finite results,
    exact zeros in y, dL_dd and dL_dlod where the row is skipped, an exact-zero dL_dd at the poles, an exact-zero dL_dlod wherever
    lod is not strictly inside (0, L-1), the model's values everywhere else, and every sentinel word unchanged."""
    dev, nan, inf = hip_device, float("nan"), float("inf")
    Cn, He, We, L = LC.SPECIAL
    g = th.Generator().manual_seed(21)
    N = 192
    base = LC.case(N, Cn, (He, We, L), "sphere", seed=3)
    d, lod = th.from_numpy(LC.directions_of(base)).clone(), th.from_numpy(LC.lod_of(base)).clone()
    skipped, poles = th.zeros(N, dtype=th.bool), th.zeros(N, dtype=th.bool)
    rows = ([0, 0, 0], [nan, 0.3, 0.2], [inf, 0.0, 1.0], [0.1, -inf, nan], [1e30, 0.0, 0.0], [-1e30, 1e30, 1e30], [nan, nan, nan], [1e-40, 0.0, -1e-41],
            [0.0, 0.0, 1.0], [0.0, 0.0, -2.5], [-0.0, 0.0, 0.7], [-1.0, 0.0, 0.3], [-2.0, -0.0, 0.6])
    below = float(np.nextafter(np.float32(L - 1), np.float32(0)))
    lods = (nan, inf, -inf, -0.0, 0.0, 1e30, -1e30, float(L - 1), below, 1.0, float(np.nextafter(np.float32(1), np.float32(0))), 1e-40)
    for k, row in enumerate(rows):
        for wave in range(3):
            r = 64 * wave + 2 * k + wave
            d[r] = th.tensor(row)
            lod[r] = nan if k < 8 else 0.3 + 0.12 * k        # (a skipped row's lod is not read)
            skipped[r], poles[r] = k < 8, 8 <= k < 11
    at = []
    for k, v in enumerate(lods):
        for wave in range(3):
            r = 64 * wave + 30 + 2 * k + wave
            lod[r] = v
            at.append(r)
    pyr = FG.envmap_pyramid(th.randn(He, We, Cn, generator=g), L)
    up = th.randn(N, Cn, generator=g)
    up[skipped] = nan                                        # (... nor its upstream)
    quiet = LC.no_dd_upstream(th.where(skipped.unsqueeze(1), th.ones(()), d).numpy(), lod.numpy(), He, We, L)
    up_d = th.where(th.from_numpy(quiet).unsqueeze(1) & ~skipped.unsqueeze(1), th.zeros(()), up)
    assert int((quiet & ~skipped.numpy()).sum()) <= 9 + LC.exclusion_cap(N)       # (the nine pole rows among them)
    y, dd, _, _ = _call_pair(_c_calls(), dev, N, Cn, (He, We, L), d, lod, pyr, up_d)
    _, _, dl, dp = _call_pair(_c_calls(), dev, N, Cn, (He, We, L), d, lod, pyr, up)
    d64 = th.where(skipped.unsqueeze(1), th.zeros(()), d).double().requires_grad_(True)
    l64, p64 = lod.double().requires_grad_(True), pyr.double().requires_grad_(True)
    y64 = FG.envmap_lod_rows(d64, l64, p64, (He, We, L))
    clean = lambda u: th.nan_to_num(u).double()
    dd64, = th.autograd.grad(y64, [d64], grad_outputs=clean(up_d), retain_graph=True)
    dl64, dp64 = th.autograd.grad(y64, [l64, p64], grad_outputs=clean(up))
    for k, a, b, tol in (("y", y, y64, FWD_TOL), ("dL_dd", dd, dd64, GRAD_TOL), ("dL_dlod", dl, dl64, GRAD_TOL), ("dL_dpyramid", dp, dp64, GRAD_TOL)):
        e = _rel(a, b.detach().numpy())
        print(f"\nspecial rows {k}: {e:.2e} (max |ref| {float(b.detach().abs().max()):.3g})")
        assert np.isfinite(a).all() and e <= tol, (k, e)
    s, p = skipped.numpy(), poles.numpy()
    assert float(np.abs(y[s]).max()) == 0.0 and float(np.abs(dd[s]).max()) == 0.0 and float(np.abs(dl[s]).max()) == 0.0 and float(np.abs(dd[p]).max()) == 0.0
    assert float(np.abs(y[p]).max(1).min()) > 0 and float(np.abs(dd[~s & ~p]).max()) > 0
    inside = np.array([0 < v < L - 1 for v in lods]).repeat(3)
    assert float(np.abs(dl[at][~inside]).max()) == 0.0 and float(np.abs(dl[at][inside]).min()) > 0
    assert np.array_equal(dl64.numpy()[at] != 0, inside)


# ---------------------------------------------------------------------------
# n_rows
# ---------------------------------------------------------------------------
def test_n_rows_on_the_device(hip_device):
    """The counts 0, below N, N, above N and negative, NaN in the tail rows of d, of lod and of the upstream: exact zeros in the
    tails of y, dL_dd and dL_dlod, dL_dpyramid the model's (nothing from the tail)."""
    c = LC.N_ROWS
    base = _inputs(c)
    for n in n_rows_counts(c.N):
        m = min(max(n, 0), c.N)
        t = dict(base, d=base["d"].clone(), lod=base["lod"].clone(), up=base["up"].clone(), up_d=base["up_d"].clone())
        t["d"][m:], t["lod"][m:], t["up"][m:], t["up_d"][m:] = float("nan"), float("nan"), float("nan"), float("nan")
        got = _run(FG.envmap_lod_rows_fused, c, t, hip_device, th.float32, n)
        clean = {k: (th.nan_to_num(v) if v.dtype.is_floating_point else v) for k, v in t.items()}
        ref = _run(FG.envmap_lod_rows, c, clean, "cpu", th.float64, n)
        within_floors(f"n_rows {n} of {c.N},", ref, got, _rel)
        assert all(float(np.abs(got[k][m:]).sum()) == 0.0 for k in ("y", "d", "l"))
        if m == 0:
            assert all(float(np.abs(got[k]).max()) == 0.0 for k in got)
        else:
            assert all(float(np.abs(got[k][:m] if k != "p" else got[k]).max()) > 0 for k in got)


# ---------------------------------------------------------------------------
# Gradient subsets
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(LC.ONLY)))
def test_only_what_is_asked(hip_device, i):
    """Each of the seven want-combinations, as one backward call, equals its part of the full call: dL_dd and dL_dlod bit for bit,
    dL_dpyramid within sum_order_tol; and the model's."""
    c, dev = LC.ONLY[i], hip_device
    t = _inputs(c)
    up = t["up_d"].to(dev)

    def backward(want):
        x = [t[k].to(dev).requires_grad_(w in want) for k, w in (("d", "d"), ("lod", "l"), ("pyr", "p"))]
        y = FG.envmap_lod_rows_fused(x[0], x[1], x[2], _spec(c))
        grads = th.autograd.grad(y, [x[GRADS[w]] for w in want], grad_outputs=up)
        return y.detach().cpu().numpy(), {w: g.cpu().numpy() for w, g in zip(want, grads)}

    y_full, full = backward("dlp")
    ref = _run(FG.envmap_lod_rows, c, dict(t, up=t["up_d"]), "cpu", th.float64, want="dlp")
    _, bounds = _models(c)
    for want in LC.WANTS:
        y, part = backward(want)
        e_p = _rel(part["p"], full["p"]) if "p" in want else 0.0
        print(f"\n{c} want {want}: " + ", ".join(f"{w} equal {np.array_equal(part[w], full[w])}" for w in want if w != "p") + (f" p {e_p:.2e} from the full call's" if "p" in want else ""))
        assert set(part) == set(want) and np.array_equal(y, y_full)
        assert all(np.array_equal(part[w], full[w]) for w in want if w != "p") and e_p <= sum_order_tol("pyramid")
        assert all(_rel(part[w], ref[w]) <= bounds[w][0] for w in want)
    x = [t[k].to(dev).detach() for k in ("d", "lod", "pyr")]
    assert not FG.envmap_lod_rows_fused(x[0], x[1], x[2], _spec(c)).requires_grad


def test_no_upstream_launches_nothing(hip_device, monkeypatch):
    """An output the loss does not use reaches the Functions' backward as None: Nones go down and the binding is not called."""
    from dmesh_renderer_amd import _C
    c = LC.ONLY[0]
    t = _inputs(c)
    d, lod = t["d"].to(hip_device).requires_grad_(True), t["lod"].to(hip_device).requires_grad_(True)
    env = th.from_numpy(LC.pyramid_base_of(c)).to(hip_device).requires_grad_(True)
    pyr = FG.envmap_pyramid_fused(env, c.L)
    y = FG.envmap_lod_rows_fused(d, lod, pyr, _spec(c))
    z = y * 1.0
    calls, builds = counts_calls(monkeypatch, _C, "envmap_lod_rows_backward"), counts_calls(monkeypatch, _C, "envmap_pyramid_backward")
    grads = th.autograd.grad((d * 3).sum() + lod.sum(), [d, lod, env], allow_unused=True)
    assert grads[2] is None and not calls and not builds
    assert FG._EnvMapLodRowsFn.backward(y.grad_fn, None) == (None,) * 7 and FG._EnvMapPyramidFn.backward(pyr.grad_fn, None) == (None, None) and not calls
    th.autograd.grad(z.sum(), [lod], retain_graph=True)
    assert calls == [1] and not builds           # dL_dlod alone: the pyramid's backward is not reached
    th.autograd.grad(z.sum(), [env])
    assert calls == [1, 1] and builds == [1]


# ---------------------------------------------------------------------------
# Against the existing unit
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(LC.AGAINST_ENVMAP)))
def test_against_the_single_level_lookup(hip_device, i):
    """At lod <= 0 (zeros, negatives, -0.0, NaN, -Inf) and, whatever lod is, at L == 1: y and dL_dd EQUAL envmap_rows_fused' on level 0
    (the same arithmetic per row: env_place(env_angles(d)) is env_coords(d), bit for bit on the host; the level of weight 0 is not
    read and adds an exact 0)."""
    c, dev = LC.AGAINST_ENVMAP[i], hip_device
    t = _inputs(c)
    lod = t["lod"].clone() if c.L == 1 else -t["lod"].abs()
    if c.L > 1:
        lod[0::5], lod[1::5], lod[2::5] = 0.0, -0.0, float("nan")
        lod[3::25] = float("-inf")
    env = t["pyr"][:c.He * c.We].reshape(c.He, c.We, c.C).to(dev)
    up = t["up_d"].to(dev)
    d0, d1 = t["d"].to(dev).requires_grad_(True), t["d"].to(dev).requires_grad_(True)
    y0 = FG.envmap_rows_fused(d0, env)
    y1 = FG.envmap_lod_rows_fused(d1, lod.to(dev), t["pyr"].to(dev), _spec(c))
    g0, = th.autograd.grad(y0, [d0], grad_outputs=up)
    g1, = th.autograd.grad(y1, [d1], grad_outputs=up)
    e_y, e_d = _rel(y1.detach().cpu().numpy(), y0.detach().cpu().numpy()), _rel(g1.cpu().numpy(), g0.cpu().numpy())
    print(f"\n{c} against envmap_rows_fused on level 0: y {e_y:.2e} (zero: {e_y == 0}), dL_dd {e_d:.2e} (zero: {e_d == 0})")
    assert e_y == 0 and e_d == 0   # (within the forward floor is what is asked; the same arithmetic on the same texels gives the same bits)


# ---------------------------------------------------------------------------
# Graph replay
# ---------------------------------------------------------------------------
def test_graph_replay(hip_device):
    """The builder, the lookup and both backwards captured into one HIP graph and replayed twice over d, lod, the base map and n_rows
    rewritten in place, the count going down and up: the stored outputs (the pyramid, y, dL_dd, dL_dlod) equal the eager ones exactly,
    the summed ones (dL_dpyramid, and dL_denvmap, which the builder's backward gathers from it) are within the gradient bound of the
    float64 model, and dL_dpyramid holds an exact zero in every texel no row touched (the rows of the rewrites lie in one half of
    the sphere)."""
    dev, c = hip_device, LC.GRAPH
    t = _inputs(c)
    d, lod = t["d"].to(dev).requires_grad_(True), t["lod"].to(dev).requires_grad_(True)
    env = th.from_numpy(LC.pyramid_base_of(c)).to(dev).requires_grad_(True)
    up, n_rows = t["up_d"].to(dev), th.tensor([500], dtype=th.int32, device=dev)
    names = ["pyr", "y", "d", "l", "p", "e"]
    zeros_checked = []

    def step():
        pyr = FG.envmap_pyramid_fused(env, c.L)
        y = FG.envmap_lod_rows_fused(d, lod, pyr, _spec(c), n_rows=n_rows)
        return [pyr.detach(), y.detach()] + list(th.autograd.grad(y, [d, lod, pyr, env], grad_outputs=up))

    def same(captured, eager, what):
        n = min(max(int(n_rows), 0), c.N)
        x64 = [v.detach().double().cpu().requires_grad_(True) for v in (d, lod, env)]
        p64 = FG.envmap_pyramid(x64[2], c.L)
        y64 = FG.envmap_lod_rows(x64[0], x64[1], p64, _spec(c), n_rows=n_rows.cpu())
        ref = dict(zip(("p", "e"), (g.numpy() for g in th.autograd.grad(y64, [p64, x64[2]], grad_outputs=up.double().cpu()))))
        touched = LC.may_touch(d.detach().cpu().numpy()[:n], lod.detach().cpu().numpy()[:n], c.He, c.We, c.L)   # (a superset: always checked)
        for name, a, b in zip(names, captured, eager):
            if name in ("pyr", "y", "d", "l"):
                print(f"\ngraph replay vs eager, {what}, {name}: equal {th.equal(a, b)}")
                assert th.equal(a, b), (what, name)
                assert name == "pyr" or (float(a[n:].abs().sum()) == 0.0 and (n == 0 or float(a[:n].abs().max()) > 0))
            else:
                e, e_ref = _rel(a.cpu().numpy(), b.cpu().numpy()), _rel(a.cpu().numpy(), ref[name])
                print(f"\ngraph replay vs eager, {what}, {name}: {e:.2e} from eager, {e_ref:.2e} from float64" + (f"; {int((~touched).sum())} texels out of every row's reach" if name == "p" else ""))
                assert e <= GRAD_TOL and e_ref <= GRAD_TOL, (what, name, e, e_ref)
                if name == "p":
                    zeros_checked.append(int((~touched).sum()))
                    assert zeros_checked[-1] > 0 and float(np.abs(a.cpu().numpy()[~touched]).sum()) == 0.0 and float(np.abs(ref["p"][~touched]).sum()) == 0.0
        assert th.equal(captured[0].cpu(), FG.envmap_pyramid(env.detach().cpu(), c.L))

    graph, captured, eager = capture_replay(step)
    for x in captured:
        x.fill_(1)
    replay(graph)
    same(captured, eager, "the captured inputs")
    g = th.Generator().manual_seed(9)
    for n, half in ((90, 1.0), (c.N, -1.0)):
        with th.no_grad():
            w = th.randn(c.N, 3, generator=g)
            w[:, 2] = half * (w[:, 2].abs() + 0.3)           # one half of the sphere: the other half of every level is not touched
            w = w / w.norm(dim=1, keepdim=True) * (0.5 + 2.5 * th.rand(c.N, 1, generator=g))
            d.copy_(w.to(dev))
            lod.copy_((th.rand(c.N, generator=g) * 3.0 - 0.5).to(dev))   # (levels 0 .. 3 of 5: the coarser ones stay untouched)
            env.copy_(th.randn(c.He, c.We, c.C, generator=g).to(dev))
            n_rows.fill_(n)
        replay(graph)
        fresh = [x.detach().clone() for x in step()]
        th.cuda.synchronize()
        same(captured, fresh, f"d, lod, the base map and n_rows = {n} rewritten in place")
    assert len(zeros_checked) == 3   # (the exact zeros were checked on the capture and on both rewrites)


# ---------------------------------------------------------------------------
# The chain of the module docstring
# ---------------------------------------------------------------------------
def test_chain_on_rendered_tri_lists(hip_device):
    """surface_packed_fused -> reflect -> EnvMapPyramid with lod from a column of a RowMLP's output, read in place -> composite_values_
    packed_fused on rendered tri lists (two views, fragment_grads=True, capacity=M), as the module docstring writes it, against the
    same chain with fragments.envmap_pyramid and envmap_lod_rows in the middle, on the device: the image, envmap.grad, the MLP's
    gradients and verts.grad, at the chain tests' bounds.  The map is turned by a generic rotation (EnvMapPyramid's frame): the scene
    is axis-aligned, so hundreds of its mirrored rays lie EXACTLY on symmetric directions (measured on these lists: 344 of 15 795
    rows with |ux| < 1e-6, 334 with |uy| < 1e-6), and those are cell lines of the coarse levels of an unturned map (665 rows within
    1e-5 texel of a cell line of the 2 x 4 level, 336 of the 1 x 2 level, none of the 8 x 16 level), where dL/dd jumps and two float32
    evaluations take either side: unturned, verts.grad differed by 7.9e-3 with four levels and 3.8e-4 with three, the image by 2.6e-7.
    The rows within 1e-5 texel of a cell line of a level they use are counted from the float64 model and printed."""
    dev, K, Hs, Ws = hip_device, 4, 72, 104
    t = {k: v.to(dev) for k, v in scenes.layered_sheets(4, 8, 2, Hs, Ws, seed=3, opacity=(0.1, 0.4)).items()}
    r = dmr.TriRenderer(dmr.TriRenderSettings(Hs, Ws, t["bg"]), return_fragments=K, fragment_grads=True)
    F = t["faces"].shape[0]
    th.manual_seed(4)
    turn, _ = th.linalg.qr(th.randn(3, 3, dtype=th.float64, generator=th.Generator().manual_seed(11)))   # orthonormal, no axis kept
    env = FG.EnvMapPyramid(8, 16, frame=turn.float()).to(dev)
    mlp = FG.RowMLP(6, 16, 4, activation="relu", out_activation="sigmoid").to(dev)
    with th.no_grad():
        env.envmap.normal_()
    assert env.levels == 4 and float(turn.abs().max()) < 0.99
    params = [env.envmap] + list(mlp.parameters())
    g_image, res = None, []
    for fused in (True, False):
        verts = t["verts"].clone().requires_grad_(True)
        frag = r(*(verts if k == "verts" else t[k] for k in TRI_ARGS))[-1]
        packed = FG.pack_slots_fused(frag, F, frag.pix_to_face.numel())
        n = packed.n_used
        s = FG.surface_packed_fused(frag, packed, t["faces"], verts, FG.camera_origins(t["mv_mats"]))
        out = mlp(th.cat([s.hit, s.normal], 1), n_rows=n)                  # [M,4]: rgb + roughness
        lod = out[:, 3] * (env.levels - 1)
        if fused:
            spec = env(s.reflect, lod, n_rows=n)
        else:
            spec = FG.envmap_lod_rows(s.reflect @ env.frame.T, lod, FG.envmap_pyramid(env.envmap, env.levels), (8, 16, env.levels), n_rows=n)
        image, T = FG.composite_values_packed_fused(frag, packed, t["faces_opacity"], out[:, :3] + spec)
        if g_image is None:
            g_image = th.randn(image.shape, generator=th.Generator().manual_seed(6)).to(dev)
        grads = th.autograd.grad((image * g_image).sum(), [verts] + params)
        res.append([image.detach().cpu().numpy()] + [g.cpu().numpy() for g in grads])
        used = int(n)
    k = LC.places64((s.reflect @ env.frame.T).detach().cpu().numpy()[:used], lod.detach().cpu().numpy()[:used], 8, 16, env.levels)
    close = ((np.minimum(np.minimum(k["fx"], 1 - k["fx"]), np.minimum(k["fy"], 1 - k["fy"])) < 1e-5) & (k["w"] != 0)).any(0) & ~k["skipped"]
    print(f"\nroughness chain: {int(close.sum())} of {used} rows within 1e-5 texel of a cell line of a level they use; lod from {float(lod[:used].detach().min()):.3f} to {float(lod[:used].detach().max()):.3f}")
    names = ["image", "verts", "envmap"] + [f"w{l}" for l in range(len(mlp.weights))] + [f"b{l}" for l in range(len(mlp.weights))]
    for k, a, b in zip(names, *res):
        e = rel_err(a, b)
        print(f"\nroughness chain ({used} rows of {packed.rows}): {k} {e:.2e} (max |ref| {float(np.abs(b).max()):.3g})")
        assert float(np.abs(b).max()) > 0 and float(np.abs(a).max()) > 0 and e <= (FWD_TOL if k == "image" else GRAD_TOL), (k, e)
