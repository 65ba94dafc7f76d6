"""fragments.envmap_rows / envmap_rows_fused / EnvMap / pixel_directions without a GPU: the model against facts that do not
come from it (a constant map, second-order convergence on a smooth function of the direction -- which a swapped or flipped axis
breaks --, agreement across the seam, gradcheck, the sum identity of the bilinear weights), pixel_directions against
tests/tri_grad_ref.py's pixel_rays, csrc/dmr_envmap_coords.hpp compiled with the host compiler and run over the bits that must
not be tried on a GPU, the library's exports and the build lists, the refusals of the functional layer and of the C ABI in their
documented order, and the case tables of the GPU tests (tests/envmap_cases.py) against the unit's dispatch."""
import math
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest
import torch as th

import envmap_cases as EC
import row_units as RU
import dmesh_renderer_amd as dmr
from dmesh_renderer_amd import fragments as FG
from row_units import CSRC, D
from tri_grad_ref import pixel_rays

UNIT_TEXT, HEADER_TEXT = RU.unit_texts("dmr_envmap.hip", "dmesh_renderer_amd_envmap.h")
COORDS_TEXT = open(os.path.join(CSRC, EC.COORDS_HEADER)).read()
FUNCTIONS = ["dmr_envmap_rows", "dmr_envmap_rows_backward"]
TORCH_PATH = r"fragments\.envmap_rows is the torch path"
NAMES = ("envmap_rows", "envmap_rows_fused", "EnvMap", "pixel_directions")


def _all_cases():
    return [c for rows in EC.tables().values() for c in rows]


def _unit_vectors(n, seed):
    d = th.randn(n, 3, dtype=th.float64, generator=th.Generator().manual_seed(seed))
    return d / d.norm(dim=1, keepdim=True)


def _centre_directions(He, We):
    """[He,We,3] float64: the direction of every texel centre, from the header: s = (j + 0.5) / We, t = (i + 0.5) / He."""
    theta = (th.arange(He, dtype=th.float64) + 0.5) / He * math.pi
    phi = ((th.arange(We, dtype=th.float64) + 0.5) / We - 0.5) * 2 * math.pi
    st, ct = theta.sin().view(He, 1), theta.cos().view(He, 1).expand(He, We)
    return th.stack([st * phi.cos().view(1, We), st * phi.sin().view(1, We), ct], -1)


# ---------------------------------------------------------------------------
# The model against independent facts
# ---------------------------------------------------------------------------
def test_a_constant_map_gives_the_constant():
    d = th.cat([_unit_vectors(500, 1) * 1.7, th.tensor([[0.0, 0.0, 2.0], [0.0, 0.0, -0.3], [-1.0, 0.0, 0.0], [-1.0, -0.0, 0.0]], dtype=th.float64)])
    for He, We in EC.MAPS:
        env = th.tensor([0.25, -3.0, 7.5], dtype=th.float64).expand(He, We, 3)
        y = FG.envmap_rows(d, env)
        assert tuple(y.shape) == (504, 3) and float((y - env[0, 0]).abs().max()) <= 1e-14, (He, We)


def test_second_order_convergence_on_a_smooth_function():
    """The map filled with the degree-2 spherical harmonics of its texel centres' directions, looked up at random directions away
    from the poles (there the lat-long rows clamp): bilinear interpolation of a smooth function is second order, so the error
    falls by about 4 when He and We double.  A transposed, flipped or shifted axis leaves an error of order 1 at every size."""
    d = _unit_vectors(4000, 2)
    d = d[d[:, 2].abs() < 0.9]
    want = FG.sh_rows(d, 3)[:, 1:]
    errs = []
    for He in (16, 32, 64, 128):
        env = FG.sh_rows(_centre_directions(He, 2 * He).reshape(-1, 3), 3)[:, 1:].reshape(He, 2 * He, 8)
        errs.append(float((FG.envmap_rows(d * 2.5, env) - want).abs().max()))
    print(f"\nlookup error of the degree-2 harmonics at He = 16, 32, 64, 128: {', '.join(f'{e:.2e}' for e in errs)}")
    assert errs[0] < 0.1 and errs[-1] < 2e-3
    for coarse, fine in zip(errs, errs[1:]):
        assert 3.0 <= coarse / fine <= 5.0, errs


def test_agreement_across_the_seam():
    """phi = +(pi - eps) and -(pi - eps) are 2 eps apart on the sphere: their lookups differ by no more than the map's slope
    allows, on a random map (columns repeat), and the exact seam (-1, +-0, 0) reads the mean of the last and the first column."""
    g = th.Generator().manual_seed(3)
    He, We, eps = 7, 13, 1e-9
    env = th.randn(He, We, 3, dtype=th.float64, generator=g)
    theta = 0.2 + (math.pi - 0.4) * th.rand(200, dtype=th.float64, generator=g)
    side = lambda phi: th.stack([theta.sin() * math.cos(phi), theta.sin() * math.sin(phi), theta.cos()], 1)
    a, b = FG.envmap_rows(side(math.pi - eps), env), FG.envmap_rows(side(-(math.pi - eps)), env)
    slope = float((env - env.roll(1, 1)).abs().max()) * We / (2 * math.pi)
    assert float((a - b).abs().max()) <= 2 * eps * slope * 1.01 + 1e-14
    row = (He - 1) // 2    # theta = pi / 2: y = He / 2 - 0.5 = 3, the centre of row 3
    for seam in ([-1.0, 0.0, 0.0], [-1.0, -0.0, 0.0]):
        y = FG.envmap_rows(th.tensor([seam], dtype=th.float64), env)[0]
        assert float((y - 0.5 * (env[row, We - 1] + env[row, 0])).abs().max()) <= 1e-12


def test_orientation_of_the_map():
    """Row 0 is +z and the last row -z; +x is the middle of a row, column 0 starts at -x and turns towards -y."""
    He, We = 4, 8
    env = th.arange(He * We, dtype=th.float64).reshape(He, We, 1)
    centres = _centre_directions(He, We)
    assert th.allclose(FG.envmap_rows(centres.reshape(-1, 3), env), env.reshape(-1, 1), rtol=0, atol=1e-12)
    assert float(centres[0, :, 2].min()) > 0.9 and float(centres[-1, :, 2].max()) < -0.9
    assert float(centres[1, 0, 0]) < 0 and float(centres[1, 0, 1]) < 0 and float(centres[1, We // 2, 0]) > 0 and float(centres[1, We // 2, 1]) > 0
    top, bottom = FG.envmap_rows(th.tensor([[0.0, 0.0, 3.0], [0.0, 0.0, -3.0]], dtype=th.float64), env)
    assert float(top) == 0.5 * (3 + 4) and float(bottom) == 0.5 * (27 + 28)   # a pole: phi = 0, between columns 3 and 4 of its row


def _away_from_cell_lines(n, He, We, seed):
    d = _unit_vectors(4 * n, seed) * (0.5 + 2.5 * th.rand(4 * n, 1, dtype=th.float64, generator=th.Generator().manual_seed(seed + 1)))
    keep = ~th.from_numpy(EC.no_dd_upstream(d.numpy(), He, We)) & th.from_numpy(EC.coords64(d.numpy(), He, We)["rho2"] > 0.05)
    return d[keep][:n].clone()


@pytest.mark.parametrize("shape", [(1, 1, 2), (1, 5, 1), (5, 1, 3), (7, 13, 4)])
def test_gradcheck(shape):
    He, We, C = shape
    d = _away_from_cell_lines(9, He, We, 4).requires_grad_(True)
    env = th.randn(He, We, C, dtype=th.float64, generator=th.Generator().manual_seed(5)).requires_grad_(True)
    assert d.shape[0] == 9
    assert th.autograd.gradcheck(lambda a, e: FG.envmap_rows(a, e), (d, env), eps=1e-7, atol=1e-6)
    n_rows = th.tensor([5])
    assert th.autograd.gradcheck(lambda a, e: FG.envmap_rows(a, e, n_rows=n_rows), (d, env), eps=1e-7, atol=1e-6)
    module = FG.EnvMap(He, We, C, frame=th.tensor([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]])).double()
    assert th.autograd.gradcheck(lambda a: module(a), (d,), eps=1e-7, atol=1e-6)


def test_the_weights_sum_to_one():
    """Per channel dL_denvmap.sum() equals the sum of the upstream over the used rows, whatever the directions are."""
    g = th.Generator().manual_seed(6)
    nan = float("nan")
    d = th.cat([_unit_vectors(300, 7) * 2, th.tensor([[0.0, 0.0, 0.0], [nan, 1.0, 0.0], [0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [1e-9, 0.0, 0.0]], dtype=th.float64)])
    used = th.ones(305, dtype=th.bool)
    used[[300, 301, 304]] = False
    for He, We in ((1, 1), (5, 1), (7, 13)):
        env = th.randn(He, We, 4, dtype=th.float64, generator=g).requires_grad_(True)
        up = th.randn(305, 4, dtype=th.float64, generator=g)
        for n in (None, 120):
            y = FG.envmap_rows(d, env, n_rows=None if n is None else th.tensor([n]))
            genv, = th.autograd.grad(y, [env], grad_outputs=up)
            rows = used if n is None else used & (th.arange(305) < n)
            assert th.allclose(genv.sum((0, 1)), up[rows].sum(0), rtol=0, atol=1e-11) and bool(th.isfinite(y).all())
            assert float(y[~rows].detach().abs().sum()) == 0.0


@pytest.mark.parametrize("dtype", [th.float32, th.float64])
def test_skipped_rows_and_poles(dtype):
    """Zero, NaN, Inf, |d| = 1e-9 (and, in float32, 1e30 and a denormal: |d|^2 leaves the format): exact zeros in y and dL/dd,
    nothing to dL/denvmap, and a NaN upstream there reaches nothing; the exact poles are read, with an exact-zero dL/dd."""
    nan, inf = float("nan"), float("inf")
    rows = [[0.0, 0.0, 0.0], [nan, 0.3, 0.2], [inf, 0.0, 1.0], [-inf, inf, nan], [0.0, 1e-9, 0.0], [0.0, 0.0, 1.0], [0.0, 0.0, -2.5], [0.3, -0.4, 0.5]]
    if dtype == th.float32:
        rows += [[1e30, 0.0, 0.0], [1e-40, 0.0, 0.0]]
    d = th.tensor(rows, dtype=dtype, requires_grad=True)
    env = th.randn(5, 9, 3, dtype=dtype, generator=th.Generator().manual_seed(8)).requires_grad_(True)
    up = th.randn(len(rows), 3, dtype=dtype, generator=th.Generator().manual_seed(9))
    skipped = [0, 1, 2, 3, 4] + list(range(8, len(rows)))
    y = FG.envmap_rows(d, env)
    gd, genv = th.autograd.grad(y, [d, env], grad_outputs=up)
    assert bool(th.isfinite(y).all() and th.isfinite(gd).all() and th.isfinite(genv).all())
    assert float(y[skipped].detach().abs().sum()) == 0.0 and float(gd[skipped].abs().sum()) == 0.0
    assert float(gd[5:7].abs().sum()) == 0.0 and float(y[5:7].detach().abs().min()) > 0 and float(gd[7].abs().max()) > 0
    assert th.allclose(genv.sum((0, 1)), up[5:8].sum(0), rtol=0, atol=1e-5)


def test_module_on_cpu_rows():
    env = FG.EnvMap(4, 8)
    assert env.out_features == 3 and tuple(env.envmap.shape) == (4, 8, 3) and [n for n, _ in env.named_parameters()] == ["envmap"] and env.frame is None
    with th.no_grad():
        env.envmap.normal_()
    d = _unit_vectors(10, 10)
    for dd in (d, d.float()):
        assert th.equal(env(dd), FG.envmap_rows(dd, env.envmap))
        assert th.equal(env(dd, n_rows=th.tensor([4]))[4:], th.zeros(6, 3, dtype=dd.dtype))
    frame = th.tensor([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]])   # the map's z axis is the world's x axis
    turned = FG.EnvMap(4, 8, 3, frame=frame)
    turned.load_state_dict(dict(env.state_dict(), frame=frame))
    assert th.allclose(turned(d.float()), FG.envmap_rows(d.float() @ frame.T, env.envmap)) and "frame" in turned.state_dict()
    assert th.allclose(turned(th.tensor([[2.0, 0.0, 0.0]])), env(th.tensor([[0.0, 0.0, 2.0]])))
    d.requires_grad_(True)
    FG.EnvMap(4, 8).double()(d).square().sum().backward()
    assert d.grad is not None
    for bad in ((0, 8, 3), (4, True, 3), (4, 8, 0), (4, 8, 17), (4.0, 8, 3)):
        with pytest.raises(ValueError, match="EnvMap: "):
            FG.EnvMap(*bad)
    with pytest.raises(ValueError, match=r"EnvMap: frame must be \[3,3\]"):
        FG.EnvMap(4, 8, 3, frame=th.eye(4))


# ---------------------------------------------------------------------------
# pixel_directions
# ---------------------------------------------------------------------------
def _cameras(B, seed):
    g = th.Generator().manual_seed(seed)
    mk = lambda: th.eye(4, dtype=th.float64).repeat(B, 1, 1) + 0.2 * th.randn(B, 4, 4, dtype=th.float64, generator=g)
    return mk(), mk()


def test_pixel_directions_are_the_pixel_rays():
    H, W = 9, 14
    mv, proj = _cameras(3, 11)
    got = FG.pixel_directions(mv, proj, H, W)
    b, py, px = th.meshgrid(th.arange(3), th.arange(H), th.arange(W), indexing="ij")
    _, ray = pixel_rays(mv, proj, b.flatten(), px.flatten(), py.flatten(), H, W)
    e = float((got.reshape(-1, 3) - ray).abs().max())
    print(f"\npixel_directions against tri_grad_ref.pixel_rays on random matrices: {e:.2e}")
    assert tuple(got.shape) == (3, H, W, 3) and got.dtype == th.float64 and e <= 1e-12
    assert float((got.norm(dim=-1) - 1).abs().max()) < 1e-5 and FG.pixel_directions(mv.float(), proj.float(), H, W).dtype == th.float32
    assert "jitter" in FG.pixel_directions.__doc__ and "NOT modelled" in FG.pixel_directions.__doc__
    for bad in ((mv[0], proj, H, W), (mv, proj[:, :3], H, W), (mv, proj[:2], H, W), (mv, proj, 0, W), (mv, proj, H, 2.0)):
        with pytest.raises(ValueError, match="pixel_directions: "):
            FG.pixel_directions(*bad)


def test_pixel_directions_gradcheck():
    mv, proj = _cameras(2, 12)
    mv.requires_grad_(True)
    proj.requires_grad_(True)
    assert th.autograd.gradcheck(lambda a, b: FG.pixel_directions(a, b, 3, 4), (mv, proj), eps=1e-6, atol=1e-7)


# ---------------------------------------------------------------------------
# dmr_envmap_coords.hpp on the host
# ---------------------------------------------------------------------------
PROGRAM = r"""
#include <cassert>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include "dmr_envmap_coords.hpp"

static long long g_calls = 0, g_modelled = 0, g_cells = 0;
static float from_bits(uint32_t b) { float f; memcpy(&f, &b, sizeof f); return f; }
static int64_t mod64(int64_t x, int64_t n) { const int64_t r = x % n; return r < 0 ? r + n : r; }
static int64_t clamp64(int64_t x, int64_t lo, int64_t hi) { return x < lo ? lo : (x > hi ? hi : x); }

// in range always; the flags by the header's float32 rule; with `model`, (x, y) and the indices against the double model
static void check(float dx, float dy, float dz, int He, int We, bool model) {
    const dmr::EnvCoords c = dmr::env_coords(dx, dy, dz, He, We);
    g_calls++;
    if (!(c.ix0 >= 0 && c.ix0 < We && c.ix1 >= 0 && c.ix1 < We && c.iy0 >= 0 && c.iy0 < He && c.iy1 >= 0 && c.iy1 < He)) {
        printf("out of range: d %a %a %a map %d x %d -> %d %d %d %d\n", dx, dy, dz, He, We, c.ix0, c.ix1, c.iy0, c.iy1);
        assert(false);
    }
    const float n = sqrtf(dx * dx + dy * dy + dz * dz);
    const bool skipped = !(n >= 1e-8f && n <= std::numeric_limits<float>::max());
    if (c.skipped != skipped) { printf("skipped: d %a %a %a -> %d, expected %d\n", dx, dy, dz, (int)c.skipped, (int)skipped); assert(false); }
    if (skipped) { assert(!c.pole); return; }
    const double X = dx, Y = dy, Z = dz, len = std::sqrt(X * X + Y * Y + Z * Z);
    const double ux = X / len, uy = Y / len, uz = Z / len, rho2 = ux * ux + uy * uy, rho = std::sqrt(rho2);
    if (rho2 < 0.5e-12) assert(c.pole);
    if (rho2 > 2e-12) assert(!c.pole);
    assert(c.fx >= 0.f && c.fx <= 1.f && c.fy >= 0.f && c.fy <= 1.f);
    if (!model || rho < 1e-6) return;
    const double pi = 3.14159265358979323846;
    const double x = (std::atan2(uy, ux) / (2 * pi) + 0.5) * We - 0.5, y = std::acos(uz < -1 ? -1 : (uz > 1 ? 1 : uz)) / pi * He - 0.5;
    // float32 rounding: u and rho carry 3 eps, atan2f 2 ulp of pi: 4e-7 of a turn's 2 pi, 6e-7 of theta's pi; twice that
    const double tol_x = (8e-7 * We) + 1e-6, tol_y = 1.2e-6 * He / pi + 1e-6;
    g_modelled++;
    // at the exact seam (-1, +-0, 0) atan2 may return either sign of pi: x is then -0.5 or We - 0.5, the same place
    double ex = std::fabs(c.x - x);
    if (std::fabs(ex - We) < ex) ex = std::fabs(ex - We);
    if (!(ex <= tol_x && std::fabs(c.y - y) <= tol_y)) {
        printf("model: d %a %a %a map %d x %d -> x %.9g y %.9g, expected %.12g %.12g (tol %.3g %.3g)\n", dx, dy, dz, He, We, c.x, c.y, x, y, tol_x, tol_y);
        assert(false);
    }
    const double fx = x - std::floor(x), fy = y - std::floor(y);
    if (fx > 2 * tol_x && fx < 1 - 2 * tol_x && fy > 2 * tol_y && fy < 1 - 2 * tol_y) {   // the cell is not in doubt: the indices are the model's
        const int64_t x0 = (int64_t)std::floor(x), y0 = (int64_t)std::floor(y);
        g_cells++;
        if (c.ix0 != mod64(x0, We) || c.ix1 != mod64(x0 + 1, We) || c.iy0 != clamp64(y0, 0, He - 1) || c.iy1 != clamp64(y0 + 1, 0, He - 1)) {
            printf("cell: d %a %a %a map %d x %d -> %d %d %d %d, x %.9g y %.9g\n", dx, dy, dz, He, We, c.ix0, c.ix1, c.iy0, c.iy1, x, y);
            assert(false);
        }
        assert(std::fabs(c.fx - fx) <= tol_x && std::fabs(c.fy - fy) <= tol_y);
    }
}

int main() {
    const int maps[5][2] = {{1, 1}, {1, 5}, {5, 1}, {7, 13}, {64, 128}};
    const float inf = std::numeric_limits<float>::infinity();
    const float hostile[] = {from_bits(0x7fc00000u), from_bits(0xffc00000u), from_bits(0x7fa00000u), from_bits(0x7fffffffu), inf, -inf, 1e30f, -1e30f,
                             3e38f, 0.f, -0.f, from_bits(0x00000001u), from_bits(0x80000001u), 1e-40f, 1e-20f, 1e-9f, -1e-9f, 1e-8f, 1.f, -1.f, 2.5f};
    const int nh = (int)(sizeof(hostile) / sizeof(hostile[0]));
    const double pi = 3.14159265358979323846;
    for (const auto& m : maps) {
        const int He = m[0], We = m[1];
        for (int i = 0; i < nh; i++)
            for (int j = 0; j < nh; j++)
                for (int k = 0; k < nh; k++) check(hostile[i], hostile[j], hostile[k], He, We, false);
        for (float s : {0.5f, 1.f, 3.f}) {   // the exact poles and the exact seam
            for (float z : {s, -s}) {
                const dmr::EnvCoords c = dmr::env_coords(0.f, 0.f, z, He, We);
                assert(!c.skipped && c.pole && c.iy0 == (z > 0 ? 0 : He - 1) && c.iy1 == c.iy0 && c.x == 0.5f * We - 0.5f);
                check(0.f, 0.f, z, He, We, false); check(-0.f, 0.f, z, He, We, false);
            }
            for (float zero : {0.f, -0.f}) {
                const dmr::EnvCoords c = dmr::env_coords(-s, zero, 0.f, He, We);
                assert(!c.skipped && !c.pole && c.ix0 == We - 1 && c.ix1 == 0 && c.fx == 0.5f);
                check(-s, zero, 0.f, He, We, true);
            }
        }
        // a dense sweep of phi and theta, the ends included, at three lengths
        for (int a = 0; a <= 720; a++)
            for (int b = 0; b <= 360; b++) {
                const double phi = -pi + 2 * pi * a / 720.0, theta = pi * b / 360.0, len = a % 3 == 0 ? 0.5 : (a % 3 == 1 ? 1.0 : 3.0);
                check((float)(len * std::sin(theta) * std::cos(phi)), (float)(len * std::sin(theta) * std::sin(phi)), (float)(len * std::cos(theta)), He, We, true);
            }
        // random bit patterns: every float there is, NaNs and denormals among them
        uint64_t s = 0x9e3779b97f4a7c15ull + (uint64_t)(He * 1000 + We);
        for (int i = 0; i < 300000; i++) {
            uint32_t w[3];
            for (int k = 0; k < 3; k++) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; w[k] = (uint32_t)(s >> 16); }
            check(from_bits(w[0]), from_bits(w[1]), from_bits(w[2]), He, We, false);
        }
    }
    printf("%lld calls, %lld against the double model, %lld cells\n", g_calls, g_modelled, g_cells);
    assert(g_modelled > 1000000 && g_cells > g_modelled / 2);
    return 0;
}
"""


def test_coords_header_on_the_host():
    """In range whatever the bits; skipped and pole as the header states them; (x, y) within float32 rounding of the double model
    and, where the cell is not in doubt, the model's indices (rows clamp, columns repeat)."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "coords.cpp"), os.path.join(tmp, "coords")
        with open(src, "w") as f:
            f.write(PROGRAM)
        subprocess.run([cxx, "-std=c++17", "-O1", "-UNDEBUG", "-ffp-contract=off", "-I", CSRC, src, "-o", exe], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
        print("\n" + out.strip())


def test_the_unit_takes_its_indices_from_that_header():
    assert '#include "%s"' % EC.COORDS_HEADER in UNIT_TEXT and '#include "dmr_texture_wrap.hpp"' in COORDS_TEXT
    for line in EC.COORDS_LINES:
        assert COORDS_TEXT.count(line) == 1, line
    assert UNIT_TEXT.count("env_coords(p.d[row * 3], p.d[row * 3 + 1], p.d[row * 3 + 2], p.He, p.We)") == 1
    assert "wrap_pair(" not in UNIT_TEXT and "floorf" not in UNIT_TEXT and "hip_runtime" not in COORDS_TEXT
    # the numpy model of tests/envmap_cases.py agrees with the torch model on the places it is used for
    d = (_unit_vectors(2000, 13) * 1.3).numpy()
    c = EC.coords64(d, 7, 13)
    env = th.arange(7 * 13, dtype=th.float64).reshape(7, 13, 1)
    mix = lambda i, j: env.numpy()[c[i], c[j], 0]
    want = (1 - c["fy"]) * ((1 - c["fx"]) * mix("iy0", "ix0") + c["fx"] * mix("iy0", "ix1")) + c["fy"] * ((1 - c["fx"]) * mix("iy1", "ix0") + c["fx"] * mix("iy1", "ix1"))
    assert float(np.abs(FG.envmap_rows(th.from_numpy(d), env)[:, 0].numpy() - want).max()) <= 1e-9


# ---------------------------------------------------------------------------
# Library, binding and build lists
# ---------------------------------------------------------------------------
def test_library_exports_the_declared_symbols():
    RU.exports_declared(HEADER_TEXT, FUNCTIONS, absent=["dmr_envmap_stats"])   # (the ablation build's counters are not in the product)


def test_the_source_and_headers_are_build_dependencies():
    RU.are_build_dependencies("dmr_envmap.hip", "dmesh_renderer_amd_envmap.h", extra=[EC.COORDS_HEADER, "dmr_texture_wrap.hpp"])


def test_binding_supports_it():
    from dmesh_renderer_amd import _C
    assert _C.SUPPORTS_FRAGMENT_ENVMAP is True and callable(_C.envmap_rows) and callable(_C.envmap_rows_backward)
    for n in NAMES:
        assert n in FG.__all__ and callable(getattr(FG, n)) and n in FG.__doc__
    assert FG._FUSED["envmap_rows"] == ("SUPPORTS_FRAGMENT_ENVMAP", "row", "environment-map lookup")
    assert FG.ENVMAP_MAX_CHANNELS == EC.MAX_C
    assert _C.ABI_VERSION == 4 and _C.NUM_STAGES == 12   # (the header adds calls, not a version)
    for line in ("env  = FG.EnvMap(256, 512).to(dev)", "dirs = FG.pixel_directions(mv_mats, proj_mats, H, W)",
                 "bg   = env(dirs.reshape(-1, 3)).view(B, H, W, 3).permute(0, 3, 1, 2)", "color = image + T * bg"):
        assert line in FG.__doc__, line
    for word in ("Mip levels", "cube maps", "a map per view", "a nearest filter", "HDR file reading"):
        assert word.lower() in HEADER_TEXT.lower(), word


# ---------------------------------------------------------------------------
# Refusals of the functional layer, with CPU tensors: nothing reaches a device
# ---------------------------------------------------------------------------
def _inputs(N=6, dtype=th.float32):
    return th.ones(N, 3, dtype=dtype), th.zeros(4, 8, 3, dtype=dtype)


def test_an_older_binding_says_rebuild(monkeypatch):
    class Old:
        SUPPORTS_FRAGMENT_SH = True

    d, env = _inputs()
    monkeypatch.setattr(dmr, "_C", Old())
    with pytest.raises(TypeError, match=r"envmap_rows_fused.*no fused row environment-map lookup: rebuild.*" + TORCH_PATH):
        FG.envmap_rows_fused(d, env)
    with pytest.raises(TypeError, match="rebuild"):   # ... before any other check
        FG.envmap_rows_fused(d[0], env[0])
    Old.SUPPORTS_FRAGMENT_ENVMAP = False
    with pytest.raises(TypeError, match="rebuild"):
        FG.envmap_rows_fused(d, env)
    assert tuple(FG.EnvMap(4, 8)(d).shape) == (6, 3)   # a CPU tensor takes the torch path: no binding needed


def test_refusals_in_their_documented_order():
    """The arguments (ValueError, both paths: d, envmap, C, an empty map, n_rows), then the fused path's dtypes and devices
    (TypeError)."""
    d, env = _inputs()
    for f, name in ((FG.envmap_rows, "envmap_rows"), (FG.envmap_rows_fused, "envmap_rows_fused")):
        with pytest.raises(ValueError, match=rf"{name}: d must be \[N,3\], got \(6, 2\)"):
            f(d[:, :2], env)
        with pytest.raises(ValueError, match=rf"{name}: d must be \[N,3\]"):
            f(d[0], env)
        with pytest.raises(ValueError, match=rf"{name}: envmap must be \[He,We,C\], got \(4, 8\)"):
            f(d, env[:, :, 0])
        with pytest.raises(ValueError, match=rf"{name}: C must be in 1..16, got 17"):
            f(d, th.zeros(4, 8, 17))
        with pytest.raises(ValueError, match=rf"{name}: C must be in 1..16, got 0"):
            f(d, env[:, :, :0])
        with pytest.raises(ValueError, match=rf"{name}: the map must have at least one texel"):
            f(d, env[:0])
        with pytest.raises(ValueError, match=rf"{name}: the map must have at least one texel"):
            f(d, env[:, :0])
        with pytest.raises(ValueError, match=rf"{name}: n_rows must be None or a tensor of one element"):
            f(d, env, n_rows=th.zeros(2, dtype=th.int32))
        with pytest.raises(ValueError, match=rf"{name}: n_rows must be None or a tensor of one element"):
            f(d, env, n_rows=3)
        with pytest.raises(ValueError, match=rf"{name}: d must be"):   # two at once: the first check wins
            f(d[0], env[0])
        with pytest.raises(ValueError, match=rf"{name}: envmap must be"):
            f(d, env[0], n_rows=3)
        with pytest.raises(ValueError, match=rf"{name}: C must be"):
            f(d, th.zeros(0, 8, 17))
    dd, ed = _inputs(dtype=th.float64)
    with pytest.raises(ValueError, match="envmap must be"):   # a bad shape and a bad dtype: the shape is refused first
        FG.envmap_rows_fused(dd, ed[0])
    with pytest.raises(TypeError, match=r"envmap_rows_fused: d must be float32, got torch.float64; " + TORCH_PATH):
        FG.envmap_rows_fused(dd, env)
    with pytest.raises(TypeError, match=r"envmap_rows_fused: envmap must be float32, got torch.float16; " + TORCH_PATH):
        FG.envmap_rows_fused(d, env.half())
    with pytest.raises(TypeError, match=r"envmap_rows_fused: n_rows must be int32, got torch.int64; " + TORCH_PATH):
        FG.envmap_rows_fused(d, env, n_rows=th.zeros(1, dtype=th.int64))
    with pytest.raises(TypeError, match=r"envmap_rows_fused: d is on cpu: every tensor must be on one HIP device.*" + TORCH_PATH):
        FG.envmap_rows_fused(d, env, n_rows=th.zeros(1, dtype=th.int32))
    for call in (lambda: dmr._C.envmap_rows(d, env, None), lambda: dmr._C.envmap_rows_backward(d, env, None, th.zeros(6, 3), True, True)):
        with pytest.raises(RuntimeError, match="no CPU path"):   # the binding below it refuses them too
            call()


# ---------------------------------------------------------------------------
# Refusals of the C ABI, through ctypes with device pointers that are never dereferenced: every check runs before any HIP call.
# No call here has wholly valid arguments and an output to write: none reaches a launch.
# ---------------------------------------------------------------------------
INTS = "N C He We"
PTRS = {"dmr_envmap_rows": "d envmap n_rows y", "dmr_envmap_rows_backward": "d envmap n_rows grad_out dL_dd dL_denvmap"}
SIZES = dict(N=1, C=3, He=4, We=8)
NULL_BY_DEFAULT = ("n_rows", "dL_dd", "dL_denvmap")
EVERY_CALL = {
    "N<0": (dict(N=-1), "bad rows"),
    "C=0": (dict(C=0), "C must be in 1..16, got 0"), "C=17": (dict(C=17), "C must be in 1..16, got 17"),
    "He=0": (dict(He=0), "the map must have at least one texel"), "We<0": (dict(We=-2), "the map must have at least one texel"),
    "too large": (dict(He=1 << 16, We=1 << 15), "map too large: He * We * ceil(C / 4) must be below 2^31"),
    "too large by the chunks": (dict(He=1 << 15, We=1 << 15, C=5), "map too large: He * We * ceil(C / 4) must be below 2^31"),
    "null d": (dict(d=None), "null d"), "null envmap": (dict(envmap=None), "null envmap"),
    # two at once: the first check wins
    "bad rows and bad C": (dict(N=-1, C=99), "bad rows"), "bad C and no texel": (dict(C=-1, He=0), "C must be in 1..16, got -1"),
    "no texel and too large": (dict(He=0, We=1 << 30), "the map must have at least one texel"),
    "too large and null d": (dict(He=1 << 16, We=1 << 15, d=None), "map too large: He * We * ceil(C / 4) must be below 2^31"),
    "null d and null envmap": (dict(d=None, envmap=None), "null d"),
}
PER_CALL = {
    "dmr_envmap_rows": {"null y": (dict(y=None), "null output"), "no rows, nothing else": (dict(N=0, d=None, envmap=None, y=None), None),
                        "null envmap and null y": (dict(envmap=None, y=None), "null envmap")},
    "dmr_envmap_rows_backward": {"null grad_out": (dict(grad_out=None), "null grad_out"), "no gradient wanted": (dict(), None),
                                 "no rows, no gradient wanted": (dict(N=0, d=None, envmap=None, grad_out=None), None),
                                 "only dL_dd wanted, no rows": (dict(N=0, d=None, envmap=None, grad_out=None, dL_dd=D), None),
                                 "bad C although no gradient wanted": (dict(C=20), "C must be in 1..16, got 20"),
                                 "null envmap and null grad_out": (dict(envmap=None, grad_out=None, dL_dd=D), "null envmap")},
}


def test_c_abi_refusals():
    import capi_ctypes
    RU.run_refusals(RU.declare(capi_ctypes.load(), FUNCTIONS), INTS, PTRS, SIZES, NULL_BY_DEFAULT, EVERY_CALL, PER_CALL)
    # the order the header documents is the order tested above
    order = re.sub(r"\s*\n \* ", " ", HEADER_TEXT[HEADER_TEXT.index("The order, for both calls"):])
    at = [order.index(w) for w in ('"bad rows"', "C,", "at least one texel", '"map too large"', "null d", "null envmap", "a null output (dmr_envmap_rows,", "null grad_out")]
    assert at == sorted(at)


# ---------------------------------------------------------------------------
# The case tables of the GPU tests
# ---------------------------------------------------------------------------
def test_dispatch_restated_as_the_unit_has_it():
    product = RU.dispatch_restated(EC, UNIT_TEXT, HEADER_TEXT, twice=EC.TWICE)
    assert [EC.via_lds(n) for n in EC.CHUNKS] == [False, True, True] and [EC.chunks_of(c) for c in (1, 4, 5, 8, 9, 12, 13, 16)] == [1, 1, 2, 2, 4, 4, 4, 4]
    # the kernels the product launches are the ones every_instantiation lists: no <NCH, !L> shape
    assert "!L>" not in product and "ablate_bits" not in product and "g_env_stats" not in product and "p.dbg" not in product and "!L>" in UNIT_TEXT


def test_the_unit_waits_for_nothing_and_zeroes_nothing_by_memset():
    code = RU.waits_for_nothing([UNIT_TEXT, COORDS_TEXT], fill_calls=1)
    # dL_dd is stored, never added: the only global atomics are the two into dL_denvmap
    assert code.count("unsafeAtomicAdd(&denv[") == 2 and code.count("unsafeAtomicAdd(") == 2 and "atomicAdd(&dd" not in code


def test_tables_reach_every_instantiation():
    full = EC.every_instantiation()
    assert len(full) == 3 + 3 + 1
    assert EC.instantiations(_all_cases()) == full
    assert EC.instantiations(EC.TABLE) == {i for i in full if i[0] != "k_envmap_rows_backward" or i[1] == (True, True)}


def test_table_holds_the_shapes_that_can_go_wrong():
    t = EC.TABLE
    assert {c.N for c in t} == {0, 1, 63, 64, 65, 255, 256, 257, 1000, EC.MAX_GROUPS * EC.THREADS + 257}
    assert {1, 3, 4, 5, 8, 16} <= {c.C for c in t} and {(c.He, c.We) for c in t} == set(EC.MAPS) and {c.layout for c in t} == set(EC.LAYOUTS)
    for n in EC.CHUNKS:   # every chunk count below and above a workgroup's tile, with float4 reads and without
        mine = [c for c in t if EC.chunks_of(c.C) == n]
        assert any(c.N <= EC.THREADS for c in mine) and any(c.N > 2 * EC.THREADS for c in mine), n
        assert any(c.C % 4 == 0 for c in mine) and (n == 4 or any(c.C % 4 for c in mine)), n
    assert {c.C for c in EC.MISALIGNED} >= {3, 4, 8, 16}
    for c in t + EC.ONLY + EC.MISALIGNED + [EC.N_ROWS, EC.GRAPH]:
        d, env = EC.directions_of(c), EC.envmap_of(c)
        assert d.shape == (c.N, 3) and d.dtype == np.float32 and env.shape == (c.He, c.We, c.C) and env.dtype == np.float32
        if c.N == 0:
            continue
        n = np.linalg.norm(d.astype(np.float64), axis=1)
        k = EC.coords64(d, c.He, c.We)
        assert n.min() > 0.49 and n.max() < 3.01 and not k["skipped"].any() and not k["pole"].any()
        share = EC.no_dd_upstream(d, c.He, c.We).mean()
        assert share <= 0.02, (c, share)   # (the GPU test asserts the same: the layouts keep the model itself below it)
        cells = len(set(zip(k["iy0"].tolist(), k["ix0"].tolist())))
        phi = np.arctan2(d[:, 1].astype(np.float64), d[:, 0])
        if c.layout == "same":
            assert cells == 1
        if c.layout == "cone" and c.N >= 255:
            assert cells <= max(9, c.N // 25)           # many rows per texel
        if c.layout == "seam":
            assert (np.pi - np.abs(phi)).max() <= 0.0501 and (c.N < 63 or ((phi > 0).any() and (phi < 0).any()))
        if c.layout == "caps":
            theta = np.arccos(np.clip(d[:, 2] / n, -1, 1))
            assert np.minimum(theta, np.pi - theta).max() <= 0.2001 and k["rho2"].min() >= 4e-4
        if c.layout == "shuffled" and c.N >= 255 and c.He >= 64:
            lanes = np.stack([k["iy0"], k["ix0"]], 1)
            assert (np.abs(np.diff(lanes, axis=0)).sum(1) > 0).mean() > 0.8   # neighbouring lanes on different texels
    big = [c for c in t if c.N > EC.MAX_GROUPS * EC.THREADS]
    assert len(big) == 2 and any(c.layout == "sphere" and c.He * c.We * ((c.C + 3) // 4) > EC.TABLE_CELLS for c in big)
