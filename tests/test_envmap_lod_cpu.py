"""fragments.envmap_pyramid / envmap_lod_rows / their fused entry points / EnvMapPyramid without a GPU: gradcheck, the models
against facts that do not come from them (the single-level lookup at integer levels, a constant map, the sum of the eight
weights, a level's texel as the mean of its base texels, the gradient of the pyramid's sums), csrc/dmr_envmap_lod_coords.hpp
compiled with the host compiler -- once plain, once with the address and undefined-behaviour sanitizers, both stand-alone
programs -- and run over the bits that must not be tried on a GPU, the library's exports and the build lists, the refusals of the
functional layer and of the C ABI in their documented order, the case tables of the GPU tests (tests/envmap_lod_cases.py) against
the unit's dispatch, and the cap on the rows a case may leave out of its dL_dd comparison."""
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest
import torch as th

import envmap_cases as EC
import envmap_lod_cases as LC
import row_units as RU
import dmesh_renderer_amd as dmr
from dmesh_renderer_amd import fragments as FG
from row_units import CSRC, D

UNIT_TEXT, HEADER_TEXT = RU.unit_texts("dmr_envmap_lod.hip", "dmesh_renderer_amd_envmap_lod.h")
COORDS_TEXT = open(os.path.join(CSRC, LC.COORDS_HEADER)).read()
BASE_COORDS_TEXT = open(os.path.join(CSRC, EC.COORDS_HEADER)).read()
FUNCTIONS = ["dmr_envmap_lod_rows", "dmr_envmap_lod_rows_backward", "dmr_envmap_pyramid", "dmr_envmap_pyramid_backward"]
TORCH_PATH = r"fragments\.envmap_lod_rows is the torch path"
NAMES = ("envmap_pyramid", "envmap_pyramid_fused", "envmap_lod_rows", "envmap_lod_rows_fused", "EnvMapPyramid")


def _all_cases():
    return [c for rows in LC.tables().values() for c in rows]


def _unit_vectors(n, seed):
    d = th.randn(n, 3, dtype=th.float64, generator=th.Generator().manual_seed(seed))
    return d / d.norm(dim=1, keepdim=True)


def _level(pyramid, spec, l):
    """level l of a pyramid as [He_l, We_l, C]"""
    He, We, L = spec
    offs, _ = LC.offsets(He, We, L)
    return pyramid[offs[l]:offs[l] + (He >> l) * (We >> l)].reshape(He >> l, We >> l, -1)


# ---------------------------------------------------------------------------
# gradcheck
# ---------------------------------------------------------------------------
def _quiet_rows(n, spec, seed):
    """n rows away from the cell lines of every level, from the poles and from integer lod -> (d, lod) float64"""
    He, We, L = spec
    g = th.Generator().manual_seed(seed)
    d = _unit_vectors(40 * n, seed) * (0.5 + 2.5 * th.rand(40 * n, 1, dtype=th.float64, generator=g))
    lod = th.rand(40 * n, dtype=th.float64, generator=g) * (L + 1) - 1          # some below 0 and above L-1: the clamps
    keep = th.from_numpy(EC.coords64(d.numpy(), He, We)["rho2"] > 0.05)
    for l in range(L):
        keep &= ~th.from_numpy(EC.no_dd_upstream(d.numpy(), He >> l, We >> l))
    keep &= ((lod - lod.round()).abs() > 0.05)
    assert int(keep.sum()) >= n
    return d[keep][:n].clone(), lod[keep][:n].clone()


@pytest.mark.parametrize("spec", [(1, 1, 1, 2), (2, 4, 2, 1), (4, 8, 3, 3), (12, 20, 3, 4)])
def test_gradcheck_of_the_lookup(spec):
    He, We, L, C = spec
    d, lod = _quiet_rows(9, (He, We, L), 4)
    _, T = LC.offsets(He, We, L)
    pyr = th.randn(T, C, dtype=th.float64, generator=th.Generator().manual_seed(5)).requires_grad_(True)   # (any [T,C] tensor in the layout)
    d.requires_grad_(True)
    lod.requires_grad_(True)
    assert th.autograd.gradcheck(lambda a, b, c: FG.envmap_lod_rows(a, b, c, (He, We, L)), (d, lod, pyr), eps=1e-7, atol=1e-6)
    n_rows = th.tensor([5])
    assert th.autograd.gradcheck(lambda a, b, c: FG.envmap_lod_rows(a, b.unsqueeze(1), c, (He, We, L), n_rows=n_rows), (d, lod, pyr), eps=1e-7, atol=1e-6)
    module = FG.EnvMapPyramid(He, We, C, L, frame=th.tensor([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]])).double()
    d2, lod2 = _quiet_rows(9, (He, We, L), 6)   # (the module turns a @ frame back into a: the rows it looks up are the quiet ones)
    assert th.autograd.gradcheck(lambda a, b: module(a @ module.frame.double(), b), (d2.requires_grad_(True), lod2.requires_grad_(True)), eps=1e-7, atol=1e-6)


@pytest.mark.parametrize("spec", [(1, 1, 1, 2), (2, 4, 2, 1), (4, 8, 3, 3), (12, 20, 3, 2)])
def test_gradcheck_of_the_builder(spec):
    He, We, L, C = spec
    env = th.randn(He, We, C, dtype=th.float64, generator=th.Generator().manual_seed(7)).requires_grad_(True)
    assert th.autograd.gradcheck(lambda e: FG.envmap_pyramid(e, L), (env,), eps=1e-6, atol=1e-7)


# ---------------------------------------------------------------------------
# Identities
# ---------------------------------------------------------------------------
def test_integer_levels_are_the_single_level_lookup():
    """L == 1, or lod <= 0 (NaN and -Inf among them), equals envmap_rows of level 0; lod = k equals envmap_rows of level k; lod at and
    above L-1 (+Inf among them) that of the top level: to 1e-12 in float64."""
    d = th.cat([_unit_vectors(300, 1) * 1.7, th.tensor([[0.0, 0.0, 2.0], [0.0, 0.0, -0.3], [-1.0, 0.0, 0.0], [-1.0, -0.0, 0.0]], dtype=th.float64)])
    N = d.shape[0]
    for He, We, L in LC.PYRAMIDS:
        env = th.randn(He, We, 3, dtype=th.float64, generator=th.Generator().manual_seed(He))
        pyr = FG.envmap_pyramid(env, L)
        at = lambda lod: FG.envmap_lod_rows(d, lod, pyr, (He, We, L))
        for lod in (th.zeros(N), th.full((N,), -0.0), th.full((N,), -3.5), th.full((N,), float("nan")), th.full((N,), float("-inf"))):
            assert float((at(lod.double()) - FG.envmap_rows(d, env)).abs().max()) <= 1e-12, (He, We, L)
        for k in range(L):
            assert float((at(th.full((N,), float(k), dtype=th.float64)) - FG.envmap_rows(d, _level(pyr, (He, We, L), k))).abs().max()) <= 1e-12, (He, We, L, k)
        for lod in (float(L - 1), L + 0.5, 1e30, float("inf")):
            assert float((at(th.full((N,), lod, dtype=th.float64)) - FG.envmap_rows(d, _level(pyr, (He, We, L), L - 1))).abs().max()) <= 1e-12
        one = FG.envmap_lod_rows(d, th.rand(N, dtype=th.float64) * 5 - 1, env.reshape(-1, 3), (He, We, 1))   # L == 1, whatever lod is
        assert float((one - FG.envmap_rows(d, env)).abs().max()) <= 1e-12


def test_between_two_levels_the_lookup_is_their_mix():
    d = _unit_vectors(200, 2) * 0.8
    He, We, L = 12, 20, 3
    pyr = FG.envmap_pyramid(th.randn(He, We, 4, dtype=th.float64, generator=th.Generator().manual_seed(3)), L)
    b = [FG.envmap_rows(d, _level(pyr, (He, We, L), k)) for k in range(L)]
    f = th.rand(200, 1, dtype=th.float64, generator=th.Generator().manual_seed(4))
    for k in range(L - 1):
        y = FG.envmap_lod_rows(d, k + f[:, 0], pyr, (He, We, L))
        assert float((y - ((1 - f) * b[k] + f * b[k + 1])).abs().max()) <= 1e-12


def test_a_constant_map_gives_the_constant_at_every_lod():
    d = _unit_vectors(300, 5) * 1.3
    for He, We, L in LC.PYRAMIDS:
        value = th.tensor([0.25, -3.0, 7.5], dtype=th.float64)
        pyr = FG.envmap_pyramid(value.expand(He, We, 3), L)
        assert float((pyr - value).abs().max()) == 0.0
        lod = th.rand(300, dtype=th.float64, generator=th.Generator().manual_seed(6)) * (L + 1) - 1
        assert float((FG.envmap_lod_rows(d, lod, pyr, (He, We, L)) - value).abs().max()) <= 1e-14


def test_the_eight_weights_sum_to_one():
    """Per channel dL_dpyramid.sum() equals the sum of the upstream over the used rows, whatever d and lod are."""
    g = th.Generator().manual_seed(6)
    nan = float("nan")
    d = th.cat([_unit_vectors(300, 7) * 2, th.tensor([[0.0, 0.0, 0.0], [nan, 1.0, 0.0], [0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [1e-9, 0.0, 0.0]], dtype=th.float64)])
    used = th.ones(305, dtype=th.bool)
    used[[300, 301, 304]] = False
    for He, We, L in ((1, 1, 1), (2, 4, 2), (12, 20, 3)):
        _, T = LC.offsets(He, We, L)
        pyr = th.randn(T, 4, dtype=th.float64, generator=g).requires_grad_(True)
        lod = th.rand(305, dtype=th.float64, generator=g) * (L + 1) - 1
        lod[300:] = nan        # (a skipped row's lod is not read; a used row's NaN is level 0)
        up = th.randn(305, 4, dtype=th.float64, generator=g)
        for n in (None, 120):
            y = FG.envmap_lod_rows(d, lod, pyr, (He, We, L), n_rows=None if n is None else th.tensor([n]))
            gp, = th.autograd.grad(y, [pyr], grad_outputs=up)
            rows = used if n is None else used & (th.arange(305) < n)
            assert th.allclose(gp.sum(0), up[rows].sum(0), rtol=0, atol=1e-11) and bool(th.isfinite(y).all())
            assert float(y[~rows].detach().abs().sum()) == 0.0


def test_a_level_is_the_mean_of_its_base_texels():
    for He, We, L in LC.PYRAMIDS:
        env = th.randn(He, We, 2, dtype=th.float64, generator=th.Generator().manual_seed(8))
        pyr = FG.envmap_pyramid(env, L)
        assert tuple(pyr.shape) == (LC.offsets(He, We, L)[1], 2) and th.equal(_level(pyr, (He, We, L), 0), env)
        for l in range(L):
            s = 1 << l
            mean = env.reshape(He // s, s, We // s, s, 2).mean((1, 3))
            assert float((_level(pyr, (He, We, L), l) - mean).abs().max()) <= 1e-12, (He, We, l)


def test_the_gradient_of_the_pyramids_sums():
    """A level holds means: a base texel has the weight 4^-l in its level-l texel.  So the gradient of the sum of level l alone is
    4^-l everywhere, that of sum(pyramid) is sum_l 4^-l, and that of the sums weighted by the texels' areas, sum_l 4^l sum(level l),
    is L everywhere."""
    for He, We, L in LC.PYRAMIDS:
        env = th.randn(He, We, 2, dtype=th.float64, generator=th.Generator().manual_seed(9)).requires_grad_(True)
        pyr = FG.envmap_pyramid(env, L)
        plain, = th.autograd.grad(pyr.sum(), [env], retain_graph=True)
        by_area, = th.autograd.grad(sum(4.0 ** l * _level(pyr, (He, We, L), l).sum() for l in range(L)), [env])
        assert float((plain - sum(4.0 ** -l for l in range(L))).abs().max()) <= 1e-12 and float((by_area - L).abs().max()) <= 1e-12


@pytest.mark.parametrize("dtype", [th.float32, th.float64])
def test_skipped_rows_poles_and_special_lod(dtype):
    """Skipped rows: exact zeros in y, dL/dd and dL/dlod, nothing to dL/dpyramid, a NaN lod or upstream there reaches nothing; the
    exact poles are read, with an exact-zero dL/dd; dL/dlod is an exact 0 wherever lod is not strictly inside (0, L-1)."""
    nan, inf = float("nan"), float("inf")
    He, We, L = 12, 20, 3
    rows = [[0.0, 0.0, 0.0], [nan, 0.3, 0.2], [inf, 0.0, 1.0], [0.0, 1e-9, 0.0], [0.0, 0.0, 1.0], [0.0, 0.0, -2.5]] + [[0.3, -0.4, 0.5]] * 9
    lods = [nan, nan, 0.5, 0.5, 0.5, 1.5] + [nan, inf, -inf, -0.0, 0.0, 1e30, 2.0, float(np.nextafter(np.float32(2), np.float32(0))), 1.0]
    d = th.tensor(rows, dtype=dtype, requires_grad=True)
    lod = th.tensor(lods, dtype=dtype, requires_grad=True)
    pyr = FG.envmap_pyramid(th.randn(He, We, 3, dtype=dtype, generator=th.Generator().manual_seed(8)), L).requires_grad_(True)
    up = th.randn(len(rows), 3, dtype=dtype, generator=th.Generator().manual_seed(9))
    y = FG.envmap_lod_rows(d, lod, pyr, (He, We, L))
    gd, gl, gp = th.autograd.grad(y, [d, lod, pyr], grad_outputs=th.where(th.arange(len(rows)).unsqueeze(1) < 4, th.full((), nan, dtype=dtype), up))
    assert bool(th.isfinite(y).all() and th.isfinite(gd).all() and th.isfinite(gl).all() and th.isfinite(gp).all())
    assert float(y[:4].detach().abs().sum()) == 0.0 and float(gd[:4].abs().sum()) == 0.0 and float(gl[:4].abs().sum()) == 0.0
    assert float(gd[4:6].abs().sum()) == 0.0 and float(y[4:6].detach().abs().min()) > 0 and float(gl[4:6].abs().min()) > 0
    inside = th.tensor([False] * 6 + [False, False, False, False, False, False, False, True, True])
    assert float(gl[6:][~inside[6:]].abs().sum()) == 0.0 and float(gl[6:][inside[6:]].abs().min()) > 0
    assert th.allclose(gp.sum(0), up[4:].sum(0), rtol=0, atol=1e-4)


def test_the_numpy_model_of_the_cases_agrees_with_the_torch_model():
    """envmap_lod_cases.places64 (written from the header) gives envmap_lod_rows' y on the places it is used for."""
    for He, We, L in LC.PYRAMIDS:
        d = (_unit_vectors(1500, 13) * 1.3).numpy()
        lod = np.random.default_rng(14).uniform(-0.5, L - 0.5, 1500).astype(np.float32)
        _, T = LC.offsets(He, We, L)
        pyr = np.random.default_rng(15).standard_normal((T, 2))
        p = LC.places64(d, lod, He, We, L)
        want = np.zeros((1500, 2))
        for k in range(2):
            ax, ay, fx, fy = 1 - p["fx"][k], 1 - p["fy"][k], p["fx"][k], p["fy"][k]
            for i, w in enumerate((ay * ax, ay * fx, fy * ax, fy * fx)):
                want += (p["w"][k] * w)[:, None] * pyr[p["rows"][k, i]]
        got = FG.envmap_lod_rows(th.from_numpy(d), th.from_numpy(lod).double(), th.from_numpy(pyr), (He, We, L)).numpy()
        assert float(np.abs(got - want).max()) <= 1e-9, (He, We, L)


def test_module_on_cpu_rows():
    env = FG.EnvMapPyramid(12, 20)
    assert env.out_features == 3 and env.levels == 3 and tuple(env.envmap.shape) == (12, 20, 3) and [n for n, _ in env.named_parameters()] == ["envmap"]
    assert env.frame is None and float(env.envmap.detach().min()) == 0.5
    assert [FG.EnvMapPyramid(h, w).levels for h, w in ((1, 1), (256, 512), (3, 8), (32, 2048), (2, 4))] == [1, 9, 1, 6, 2]
    assert FG.EnvMapPyramid(16, 32, 4, levels=2).levels == 2 and FG.EnvMapPyramid(2048, 4096, 1).levels == 12   # (up to 12)
    with th.no_grad():
        env.envmap.normal_()
    d, lod = _unit_vectors(10, 10), th.rand(10, dtype=th.float64) * 2
    for dd, ll in ((d, lod), (d.float(), lod.float())):
        want = FG.envmap_lod_rows(dd, ll, FG.envmap_pyramid(env.envmap, 3), (12, 20, 3))
        assert th.equal(env(dd, ll), want) and th.equal(env(dd, ll.unsqueeze(1)), want)
        assert th.equal(env(dd, ll, n_rows=th.tensor([4]))[4:], th.zeros(6, 3, dtype=dd.dtype))
    frame = th.tensor([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]])
    turned = FG.EnvMapPyramid(12, 20, 3, frame=frame)
    turned.load_state_dict(dict(env.state_dict(), frame=frame))
    assert th.allclose(turned(d.float(), lod.float()), env(d.float() @ frame.T, lod.float())) and "frame" in turned.state_dict()
    d.requires_grad_(True)
    lod.requires_grad_(True)
    m = FG.EnvMapPyramid(12, 20).double()
    with th.no_grad():
        m.envmap.normal_()
    m(d, lod).square().sum().backward()
    assert d.grad is not None and lod.grad is not None and int((m.envmap.grad != 0).any(2).sum()) > 4 * 10   # (through the pyramid: more base texels than level 0 alone gives)
    for bad in ((0, 8, 3), (4, True, 3), (4, 8, 0), (4, 8, 17), (4.0, 8, 3), (12, 20, 3, 4), (12, 20, 3, 0), (12, 20, 3, 13), (8, 8, 3, 2.0)):
        with pytest.raises(ValueError, match="EnvMapPyramid: "):
            FG.EnvMapPyramid(*bad)
    with pytest.raises(ValueError, match=r"EnvMapPyramid: frame must be \[3,3\]"):
        FG.EnvMapPyramid(4, 8, 3, frame=th.eye(4))


# ---------------------------------------------------------------------------
# dmr_envmap_lod_coords.hpp on the host: one program, built plain and built with the sanitizers
# ---------------------------------------------------------------------------
PROGRAM = r"""
#include <cassert>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include "dmr_envmap_lod_coords.hpp"

static long long g_calls = 0, g_placed = 0;
static float from_bits(uint32_t b) { float f; memcpy(&f, &b, sizeof f); return f; }
static uint32_t bits_of(float f) { uint32_t b; memcpy(&b, &f, sizeof b); return b; }
static bool same(float a, float b) { return bits_of(a) == bits_of(b); }
static uint32_t next(uint64_t& s) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (uint32_t)(s >> 16); }

// env_place(env_angles(d), He, We) == env_coords(d, He, We), field by field and bit for bit; its indices in range
static void check(float dx, float dy, float dz, int He, int We) {
    const dmr::EnvCoords c = dmr::env_coords(dx, dy, dz, He, We);
    const dmr::EnvAngles a = dmr::env_angles(dx, dy, dz);
    g_calls++;
    if (a.skipped != c.skipped) { printf("skipped: d %a %a %a\n", dx, dy, dz); assert(false); }
    if (a.skipped) { assert(!a.pole && a.s == 0.f && a.t == 0.f); return; }
    const dmr::EnvPlace p = dmr::env_place(a.s, a.t, He, We);
    g_placed++;
    const bool fields = a.pole == c.pole && same(a.ux, c.ux) && same(a.uy, c.uy) && same(a.uz, c.uz) && same(a.inv, c.inv) && same(a.rho2, c.rho2) &&
                        same(p.x, c.x) && same(p.y, c.y) && same(p.fx, c.fx) && same(p.fy, c.fy);
    const bool indices = p.ix0 == c.ix0 && p.ix1 == c.ix1 && p.iy0 == c.iy0 && p.iy1 == c.iy1;
    if (!fields || !indices) {
        printf("differs: d %a %a %a map %d x %d: x %a %a y %a %a indices %d %d %d %d / %d %d %d %d\n", dx, dy, dz, He, We, p.x, c.x, p.y, c.y,
               p.ix0, p.ix1, p.iy0, p.iy1, c.ix0, c.ix1, c.iy0, c.iy1);
        assert(false);
    }
    assert(p.ix0 >= 0 && p.ix0 < We && p.ix1 >= 0 && p.ix1 < We && p.iy0 >= 0 && p.iy0 < He && p.iy1 >= 0 && p.iy1 < He);
}

static int place_sweep() {
    const int maps[7][2] = {{1, 1}, {1, 5}, {5, 1}, {7, 13}, {12, 20}, {3, 5}, {64, 128}};
    const float inf = std::numeric_limits<float>::infinity();
    const float hostile[] = {from_bits(0x7fc00000u), from_bits(0xffc00000u), from_bits(0x7fa00000u), from_bits(0x7fffffffu), inf, -inf, 1e30f, -1e30f,
                             3e38f, 0.f, -0.f, from_bits(0x00000001u), from_bits(0x80000001u), 1e-40f, 1e-20f, 1e-9f, -1e-9f, 1e-8f, 1.f, -1.f, 2.5f};
    const int nh = (int)(sizeof(hostile) / sizeof(hostile[0]));
    const double pi = 3.14159265358979323846;
    for (const auto& m : maps) {
        const int He = m[0], We = m[1];
        for (int i = 0; i < nh; i++)
            for (int j = 0; j < nh; j++)
                for (int k = 0; k < nh; k++) check(hostile[i], hostile[j], hostile[k], He, We);
        for (float s : {0.5f, 1.f, 3.f}) {   // the exact poles and the exact seam
            for (float z : {s, -s}) { check(0.f, 0.f, z, He, We); check(-0.f, 0.f, z, He, We); }
            for (float zero : {0.f, -0.f}) check(-s, zero, 0.f, He, We);
        }
        for (int a = 0; a <= 720; a++)   // a dense sweep of phi and theta, the ends included, at three lengths
            for (int b = 0; b <= 360; b++) {
                const double phi = -pi + 2 * pi * a / 720.0, theta = pi * b / 360.0, len = a % 3 == 0 ? 0.5 : (a % 3 == 1 ? 1.0 : 3.0);
                check((float)(len * std::sin(theta) * std::cos(phi)), (float)(len * std::sin(theta) * std::sin(phi)), (float)(len * std::cos(theta)), He, We);
            }
        uint64_t s = 0x9e3779b97f4a7c15ull + (uint64_t)(He * 1000 + We);
        for (int i = 0; i < 300000; i++) {   // random bit patterns of d: every float there is ...
            const float x = from_bits(next(s)), y = from_bits(next(s)), z = from_bits(next(s));
            check(x, y, z, He, We);
        }
        for (int i = 0; i < 300000; i++) {   // ... and of (s, t) themselves: in range whatever they hold
            const dmr::EnvPlace p = dmr::env_place(from_bits(next(s)), from_bits(next(s)), He, We);
            assert(p.ix0 >= 0 && p.ix0 < We && p.ix1 >= 0 && p.ix1 < We && p.iy0 >= 0 && p.iy0 < He && p.iy1 >= 0 && p.iy1 < He);
        }
    }
    // a level's offset is the sum of the levels below it
    long long specs = 0;
    for (int L = 1; L <= dmr::ENV_LOD_MAX_LEVELS; L++)
        for (int h = 1; h <= 5; h++)
            for (int w = 1; w <= 7; w++) {
                const int He = h << (L - 1), We = w << (L - 1);
                uint64_t off = 0;
                for (int l = 0; l < L; l++) {
                    if (off >= (1ull << 31)) break;
                    assert(dmr::env_lod_offset(He, We, l) == (uint32_t)off);
                    off += (uint64_t)(He >> l) * (uint64_t)(We >> l);
                    specs++;
                }
            }
    printf("%lld calls, %lld placed, %lld offsets\n", g_calls, g_placed, specs);
    assert(g_calls > 3000000 && g_placed > 1000000);
    return 0;
}

// every special value, every integer and half-integer up to 12, the neighbours of each, 1e6 random bit patterns: the ranges here,
// one 12-byte record per lod on stdout for the numpy model
static int level_sweep(int L) {
    struct Record { uint32_t bits; int8_t l0, l1, inside, pad; float f; };
    static_assert(sizeof(Record) == 12, "");
    const float inf = std::numeric_limits<float>::infinity();
    uint64_t s = 0x2545f4914f6cdd1dull + (uint64_t)L;
    const float special[] = {from_bits(0x7fc00000u), from_bits(0xffc00000u), from_bits(0x7fa00000u), inf, -inf, 0.f, -0.f, 1e30f, -1e30f, 3e38f,
                             from_bits(0x00000001u), from_bits(0x80000001u), 1e-40f, 1e-20f, -1e-20f};
    long long n = 0;
    const auto one = [&](float lod) {
        const dmr::EnvLodLevels v = dmr::env_lod_levels(lod, L);
        if (!(0 <= v.l0 && v.l0 <= v.l1 && v.l1 <= L - 1 && v.f >= 0.f && v.f <= 1.f && (L > 1 || (v.f == 0.f && !v.inside)))) {
            fprintf(stderr, "range: lod %a L %d -> %d %d %a\n", lod, L, v.l0, v.l1, v.f);
            assert(false);
        }
        const Record r = {bits_of(lod), (int8_t)v.l0, (int8_t)v.l1, (int8_t)v.inside, 0, v.f};
        fwrite(&r, sizeof r, 1, stdout);
        n++;
    };
    for (float x : special) one(x);
    for (int i = -2; i <= 26; i++) {
        const float x = 0.5f * (float)i;
        one(x); one(std::nextafter(x, inf)); one(std::nextafter(x, -inf)); one(-x);
    }
    for (int i = 0; i < 1000000; i++) one(from_bits(next(s)));
    for (int i = 0; i < 200000; i++) one((float)((double)next(s) / 4294967296.0 * 14.0 - 1.0));   // ... and where the levels are
    fprintf(stderr, "L %d: %lld values\n", L, n);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "place")) return place_sweep();
    if (argc == 3 && !strcmp(argv[1], "levels")) return level_sweep(atoi(argv[2]));
    return 2;
}
"""


def _build_program(tmp, name, extra):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    src, exe = os.path.join(tmp, "lod_coords.cpp"), os.path.join(tmp, name)
    with open(src, "w") as f:
        f.write(PROGRAM)
    subprocess.run([cxx, "-std=c++17", "-O1", "-UNDEBUG", "-ffp-contract=off", *extra, "-I", CSRC, src, "-o", exe], check=True)
    return exe


def _run_program(exe, check_levels):
    """The placement sweep, then the level sweep for every L in 1..12 (check_levels: its records against the numpy model)."""
    out = subprocess.run([exe, "place"], check=True, capture_output=True, text=True).stdout
    print("\n" + out.strip())
    record = np.dtype([("bits", "<u4"), ("l0", "i1"), ("l1", "i1"), ("inside", "i1"), ("pad", "i1"), ("f", "<f4")])
    for L in range(1, LC.MAX_L + 1):
        raw = subprocess.run([exe, "levels", str(L)], check=True, capture_output=True).stdout
        r = np.frombuffer(raw, dtype=record)
        assert r.shape[0] > 1200000
        if not check_levels:
            continue
        lod = r["bits"].view(np.float32)
        assert (0 <= r["l0"]).all() and (r["l0"] <= r["l1"]).all() and (r["l1"] <= L - 1).all() and (r["f"] >= 0).all() and (r["f"] <= 1).all()
        fin = np.isfinite(lod)
        l0, l1, f, inside = LC.levels64(lod[fin], L)
        assert fin.sum() > 1100000 and np.array_equal(r["l0"][fin], l0) and np.array_equal(r["l1"][fin], l1), L
        assert np.array_equal(r["f"][fin].astype(np.float64), f) and np.array_equal(r["inside"][fin] != 0, inside), L
        # what is not finite: a NaN and -Inf are level 0, +Inf the top level; none is inside
        nan, pinf = np.isnan(lod), lod == np.inf
        assert (r["l0"][nan] == 0).all() and (r["f"][nan] == 0).all() and (r["inside"][~fin] == 0).all()
        assert (r["l1"][pinf] == L - 1).all() and (r["f"][pinf] == (1 if L > 1 else 0)).all()


def test_coords_header_on_the_host():
    """env_place(env_angles(d), He, We) equals env_coords(d, He, We) bit for bit, fields and indices alike, on hostile values, the
    exact poles and seam, a dense sweep and 2.1e6 random bit patterns; env_lod_levels over every special value, every integer and
    half-integer up to 12 and 1e6 random bit patterns for every L in 1..12: 0 <= l0 <= l1 <= L-1, 0 <= f <= 1, and the numpy model's
    (envmap_lod_cases.levels64) levels, fraction and `inside` wherever lod is finite."""
    with tempfile.TemporaryDirectory() as tmp:
        _run_program(_build_program(tmp, "lod_coords", []), check_levels=True)


def test_coords_header_on_the_host_under_the_sanitizers():
    """The same program built with -fsanitize=address,undefined and float-cast-overflow (stand-alone: no Python in the process, nothing preloaded) runs the
    same sweeps to the end: no out-of-range conversion, no overflow, no bad access."""
    with tempfile.TemporaryDirectory() as tmp:
        exe = _build_program(tmp, "lod_coords_san", ["-g", "-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=all"])
        _run_program(exe, check_levels=False)


def test_the_unit_takes_its_levels_and_texels_from_that_header():
    assert '#include "%s"' % LC.COORDS_HEADER in UNIT_TEXT and '#include "%s"' % EC.COORDS_HEADER in COORDS_TEXT
    for line in LC.COORDS_LINES:
        assert COORDS_TEXT.count(line) == 1, line
    assert UNIT_TEXT.count("env_angles(p.d[row * 3], p.d[row * 3 + 1], p.d[row * 3 + 2])") == 1
    assert UNIT_TEXT.count("env_lod_levels(p.lod[row * p.lod_stride], p.L)") == 1 and UNIT_TEXT.count("env_place(a.s, a.t, r.He[k], r.We[k])") == 1
    code = re.sub(r"//[^\n]*", "", UNIT_TEXT)
    assert all(w not in code for w in ("wrap_pair(", "floorf", "atan2f", "env_coords(")) and "hip_runtime" not in COORDS_TEXT
    assert "env_lod" not in BASE_COORDS_TEXT   # (the existing header is included, not edited)


# ---------------------------------------------------------------------------
# Library, binding and build lists
# ---------------------------------------------------------------------------
def test_library_exports_the_declared_symbols():
    RU.exports_declared(HEADER_TEXT, FUNCTIONS, absent=["dmr_envmap_lod_stats"])   # (the ablation build's counters are not in the product)


def test_the_source_and_headers_are_build_dependencies():
    RU.are_build_dependencies("dmr_envmap_lod.hip", "dmesh_renderer_amd_envmap_lod.h", extra=[LC.COORDS_HEADER, EC.COORDS_HEADER, "dmr_texture_wrap.hpp"])


def test_binding_supports_it():
    from dmesh_renderer_amd import _C
    assert _C.SUPPORTS_FRAGMENT_ENVMAP_LOD is True
    assert all(callable(getattr(_C, n)) for n in ("envmap_pyramid", "envmap_pyramid_backward", "envmap_lod_rows", "envmap_lod_rows_backward"))
    for n in NAMES:
        assert n in FG.__all__ and callable(getattr(FG, n)) and n in FG.__doc__
    assert FG._FUSED["envmap_lod_rows"][:2] == ("SUPPORTS_FRAGMENT_ENVMAP_LOD", "row") and FG._FUSED["envmap_pyramid"][:2] == ("SUPPORTS_FRAGMENT_ENVMAP_LOD", "row")
    assert FG.ENVMAP_LOD_MAX_LEVELS == LC.MAX_L and FG.ENVMAP_MAX_CHANNELS == LC.MAX_C
    assert _C.ABI_VERSION == 4 and _C.NUM_STAGES == 12   # (the header adds calls, not a version)
    for line in ("env = FG.EnvMapPyramid(256, 512).to(dev)", "spec = env(s.reflect, out[:, 3].sigmoid() * (env.levels - 1), n_rows=n)",
                 "image, T = FG.composite_values_packed_fused(frag, packed, faces_opacity, out[:, :3] + spec)"):
        assert line in FG.__doc__, line
    for text in (HEADER_TEXT, FG.envmap_pyramid.__doc__):   # what the builder is, and that the lookup takes any pyramid in the layout
        flat = re.sub(r"\s*\n \* |\s*\n\s*", " ", text)
        assert "BOX mip chain" in flat and "NOT a solid-angle or GGX prefilter" in flat and "prefiltered elsewhere" in flat
    assert FG._pyramid_spec("t", 12, 20, 3, 3) == LC.offsets(12, 20, 3)


# ---------------------------------------------------------------------------
# Refusals of the functional layer, with CPU tensors: nothing reaches a device
# ---------------------------------------------------------------------------
def _inputs(N=6, dtype=th.float32):
    return th.ones(N, 3, dtype=dtype), th.zeros(N, dtype=dtype), th.zeros(LC.offsets(4, 8, 3)[1], 3, dtype=dtype)


def test_an_older_binding_says_rebuild(monkeypatch):
    class Old:
        SUPPORTS_FRAGMENT_ENVMAP = True

    d, lod, pyr = _inputs()
    monkeypatch.setattr(dmr, "_C", Old())
    with pytest.raises(TypeError, match=r"envmap_lod_rows_fused.*no fused row environment-map lookup by level of detail: rebuild.*" + TORCH_PATH):
        FG.envmap_lod_rows_fused(d, lod, pyr, (4, 8, 3))
    with pytest.raises(TypeError, match=r"envmap_pyramid_fused.*no fused row environment-map pyramid: rebuild.*fragments\.envmap_pyramid is the torch path"):
        FG.envmap_pyramid_fused(th.zeros(4, 8, 3), 3)
    with pytest.raises(TypeError, match="rebuild"):   # ... before any other check
        FG.envmap_lod_rows_fused(d[0], lod, pyr, (4, 8, 3))
    Old.SUPPORTS_FRAGMENT_ENVMAP_LOD = False
    with pytest.raises(TypeError, match="rebuild"):
        FG.envmap_lod_rows_fused(d, lod, pyr, (4, 8, 3))
    assert tuple(FG.EnvMapPyramid(4, 8)(d, lod).shape) == (6, 3)   # a CPU tensor takes the torch path: no binding needed


def test_refusals_in_their_documented_order():
    """The arguments (ValueError, both paths: d, lod, pyramid, levels, C, L, an empty map, the multiples, the pyramid's rows, n_rows),
    then the fused path's dtypes and devices (TypeError); the builder alike."""
    d, lod, pyr = _inputs()
    spec = (4, 8, 3)
    for f, name in ((FG.envmap_lod_rows, "envmap_lod_rows"), (FG.envmap_lod_rows_fused, "envmap_lod_rows_fused")):
        with pytest.raises(ValueError, match=rf"{name}: d must be \[N,3\], got \(6, 2\)"):
            f(d[:, :2], lod, pyr, spec)
        with pytest.raises(ValueError, match=rf"{name}: lod must be \[N\] or \[N,1\] = \(6,\), got \(5,\)"):
            f(d, lod[:5], pyr, spec)
        with pytest.raises(ValueError, match=rf"{name}: lod must be"):
            f(d, lod.view(6, 1, 1), pyr, spec)
        with pytest.raises(ValueError, match=rf"{name}: pyramid must be \[T,C\], got \(4, 8, 3\)"):
            f(d, lod, th.zeros(4, 8, 3), spec)
        with pytest.raises(ValueError, match=rf"{name}: levels must be the spec \(He, We, L\), got 3"):
            f(d, lod, pyr, 3)
        with pytest.raises(ValueError, match=rf"{name}: C must be in 1..16, got 17"):
            f(d, lod, th.zeros(42, 17), spec)
        with pytest.raises(ValueError, match=rf"{name}: levels must be an int in 1..12"):
            f(d, lod, pyr, (4, 8, 0))
        with pytest.raises(ValueError, match=rf"{name}: levels must be an int in 1..12"):
            f(d, lod, pyr, (4, 8, 13))
        with pytest.raises(ValueError, match=rf"{name}: levels must be an int in 1..12"):
            f(d, lod, pyr, (4.0, 8, 3))
        with pytest.raises(ValueError, match=rf"{name}: the map must have at least one texel"):
            f(d, lod, pyr, (0, 8, 3))
        with pytest.raises(ValueError, match=rf"{name}: He and We must be multiples of 2\^\(levels-1\) = 4, got \(6, 8\)"):
            f(d, lod, pyr, (6, 8, 3))
        with pytest.raises(ValueError, match=rf"{name}: T \* ceil\(C / 4\) must be below 2\^31"):
            f(d, lod, pyr, (1 << 16, 1 << 15, 1))
        with pytest.raises(ValueError, match=rf"{name}: pyramid must have the T = 40 rows of the spec \(4, 8, 2\), got \(42, 3\)"):
            f(d, lod, pyr, (4, 8, 2))
        with pytest.raises(ValueError, match=rf"{name}: n_rows must be None or a tensor of one element"):
            f(d, lod, pyr, spec, n_rows=th.zeros(2, dtype=th.int32))
        with pytest.raises(ValueError, match=rf"{name}: d must be"):   # two at once: the first check wins
            f(d[0], lod[:2], pyr, spec)
        with pytest.raises(ValueError, match=rf"{name}: lod must be"):
            f(d, lod[:2], pyr[0], spec)
        with pytest.raises(ValueError, match=rf"{name}: C must be"):
            f(d, lod, th.zeros(42, 17), (4, 8, 0))
        with pytest.raises(ValueError, match=rf"{name}: pyramid must have"):
            f(d, lod, pyr[:40], spec, n_rows=3)
    d64, lod64, pyr64 = _inputs(dtype=th.float64)
    with pytest.raises(ValueError, match="pyramid must be"):   # a bad shape and a bad dtype: the shape is refused first
        FG.envmap_lod_rows_fused(d64, lod64, pyr64[0], spec)
    with pytest.raises(TypeError, match=r"envmap_lod_rows_fused: d must be float32, got torch.float64; " + TORCH_PATH):
        FG.envmap_lod_rows_fused(d64, lod, pyr, spec)
    with pytest.raises(TypeError, match=r"envmap_lod_rows_fused: lod must be float32, got torch.float64; " + TORCH_PATH):
        FG.envmap_lod_rows_fused(d, lod64, pyr, spec)
    with pytest.raises(TypeError, match=r"envmap_lod_rows_fused: pyramid must be float32, got torch.float16; " + TORCH_PATH):
        FG.envmap_lod_rows_fused(d, lod, pyr.half(), spec)
    with pytest.raises(TypeError, match=r"envmap_lod_rows_fused: n_rows must be int32, got torch.int64; " + TORCH_PATH):
        FG.envmap_lod_rows_fused(d, lod, pyr, spec, n_rows=th.zeros(1, dtype=th.int64))
    with pytest.raises(TypeError, match=r"envmap_lod_rows_fused: d is on cpu: every tensor must be on one HIP device.*" + TORCH_PATH):
        FG.envmap_lod_rows_fused(d, lod, pyr, spec, n_rows=th.zeros(1, dtype=th.int32))
    env = th.zeros(4, 8, 3)
    for f, name in ((FG.envmap_pyramid, "envmap_pyramid"), (FG.envmap_pyramid_fused, "envmap_pyramid_fused")):
        with pytest.raises(ValueError, match=rf"{name}: envmap must be \[He,We,C\], got \(4, 8\)"):
            f(env[:, :, 0], 3)
        with pytest.raises(ValueError, match=rf"{name}: C must be in 1..16, got 17"):
            f(th.zeros(4, 8, 17), 3)
        with pytest.raises(ValueError, match=rf"{name}: levels must be an int in 1..12"):
            f(env, 0)
        with pytest.raises(ValueError, match=rf"{name}: levels must be an int in 1..12"):
            f(env, True)
        with pytest.raises(ValueError, match=rf"{name}: the map must have at least one texel"):
            f(env[:0], 1)
        with pytest.raises(ValueError, match=rf"{name}: He and We must be multiples of 2\^\(levels-1\) = 8, got \(4, 8\)"):
            f(env, 4)
        with pytest.raises(ValueError, match=rf"{name}: C must be"):   # two at once: the first check wins
            f(th.zeros(4, 8, 17), 9)
    with pytest.raises(TypeError, match=r"envmap_pyramid_fused: envmap must be float32, got torch.float64; fragments\.envmap_pyramid is the torch path"):
        FG.envmap_pyramid_fused(env.double(), 3)
    with pytest.raises(TypeError, match=r"envmap_pyramid_fused: envmap is on cpu: every tensor must be on one HIP device"):
        FG.envmap_pyramid_fused(env, 3)
    calls = (lambda: dmr._C.envmap_pyramid(env, 3), lambda: dmr._C.envmap_pyramid_backward(pyr, 4, 8, 3), lambda: dmr._C.envmap_lod_rows(d, lod, pyr, 4, 8, 3, None),
             lambda: dmr._C.envmap_lod_rows_backward(d, lod, pyr, 4, 8, 3, None, th.zeros(6, 3), True, True, True))
    for call in calls:
        with pytest.raises(RuntimeError, match="no CPU path"):   # the binding below it refuses them too
            call()


# ---------------------------------------------------------------------------
# Refusals of the C ABI, through ctypes with device pointers that are never dereferenced: every check runs before any HIP call.
# No call here has wholly valid arguments and an output to write: none reaches a launch.
# ---------------------------------------------------------------------------
TOO_LARGE = "pyramid too large: T * ceil(C / 4) must be below 2^31"
MULTIPLES = "He and We must be multiples of 2^(L-1)"
SPEC_REFUSALS = {
    "C=0": (dict(C=0), "C must be in 1..16, got 0"), "C=17": (dict(C=17), "C must be in 1..16, got 17"),
    "L=0": (dict(L=0), "L must be in 1..12, got 0"), "L=13": (dict(L=13), "L must be in 1..12, got 13"),
    "He=0": (dict(He=0), "the map must have at least one texel"), "We<0": (dict(We=-4), "the map must have at least one texel"),
    "He no multiple": (dict(He=6), MULTIPLES), "We no multiple": (dict(We=10), MULTIPLES), "one level more": (dict(L=4), MULTIPLES),
    "too large": (dict(He=1 << 16, We=1 << 15, L=1), TOO_LARGE), "too large by the chunks": (dict(He=1 << 15, We=1 << 15, C=5, L=1), TOO_LARGE),
    "too large by the levels": (dict(He=46336, We=46336, L=2), TOO_LARGE),   # (the base alone is 2 147 024 896 texels: below 2^31; with level 1 above it)
    # two at once: the first check wins
    "bad C and bad L": (dict(C=-1, L=0), "C must be in 1..16, got -1"), "bad L and no texel": (dict(L=99, He=0), "L must be in 1..12, got 99"),
    "no texel and no multiple": (dict(He=0, We=10), "the map must have at least one texel"),
    "no multiple and too large": (dict(He=(1 << 16) + 2, We=1 << 16), MULTIPLES),
}
LOOKUP_INTS, BUILDER_INTS = "N C He We L lod_stride", "C He We L"
LOOKUP_PTRS = {"dmr_envmap_lod_rows": "d lod pyramid n_rows y", "dmr_envmap_lod_rows_backward": "d lod pyramid n_rows grad_out dL_dd dL_dlod dL_dpyramid"}
BUILDER_PTRS = {"dmr_envmap_pyramid": "envmap pyramid", "dmr_envmap_pyramid_backward": "grad_pyramid dL_denvmap"}
SIZES = dict(N=1, C=3, He=4, We=8, L=3, lod_stride=1)
NULL_BY_DEFAULT = ("n_rows", "dL_dd", "dL_dlod", "dL_dpyramid")
LOOKUP_EVERY_CALL = dict(SPEC_REFUSALS, **{
    "N<0": (dict(N=-1), "bad rows"), "bad rows and bad C": (dict(N=-1, C=99), "bad rows"),
    "stride 0": (dict(lod_stride=0), "lod_stride must be at least 1"), "stride<0": (dict(lod_stride=-4), "lod_stride must be at least 1"),
    "null d": (dict(d=None), "null d"), "null lod": (dict(lod=None), "null lod"), "null pyramid": (dict(pyramid=None), "null pyramid"),
    "too large and bad stride": (dict(He=1 << 16, We=1 << 15, L=1, lod_stride=0), TOO_LARGE),
    "bad stride and null d": (dict(lod_stride=0, d=None), "lod_stride must be at least 1"),
    "null d and null lod": (dict(d=None, lod=None), "null d"), "null lod and null pyramid": (dict(lod=None, pyramid=None), "null lod"),
})
NO_ROWS = dict(N=0, d=None, lod=None, pyramid=None)
LOOKUP_PER_CALL = {
    "dmr_envmap_lod_rows": {"null y": (dict(y=None), "null output"), "no rows, nothing else": (dict(NO_ROWS, y=None), None),
                            "null pyramid and null y": (dict(pyramid=None, y=None), "null pyramid")},
    "dmr_envmap_lod_rows_backward": {"null grad_out": (dict(grad_out=None), "null grad_out"), "no gradient wanted": (dict(), None),
                                     "no rows, no gradient wanted": (dict(NO_ROWS, grad_out=None), None),
                                     "only dL_dd wanted, no rows": (dict(NO_ROWS, grad_out=None, dL_dd=D), None),
                                     "only dL_dlod wanted, no rows": (dict(NO_ROWS, grad_out=None, dL_dlod=D), None),
                                     "bad L although no gradient wanted": (dict(L=20), "L must be in 1..12, got 20"),
                                     "null pyramid and null grad_out": (dict(pyramid=None, grad_out=None, dL_dlod=D), "null pyramid")},
}
BUILDER_PER_CALL = {
    "dmr_envmap_pyramid": {"null envmap": (dict(envmap=None), "null envmap"), "null pyramid": (dict(pyramid=None), "null output"),
                           "both null": (dict(envmap=None, pyramid=None), "null envmap"), "bad C and null envmap": (dict(C=0, envmap=None), "C must be in 1..16, got 0")},
    "dmr_envmap_pyramid_backward": {"null grad_pyramid": (dict(grad_pyramid=None), "null grad_pyramid"), "null dL_denvmap": (dict(dL_denvmap=None), "null output"),
                                    "both null": (dict(grad_pyramid=None, dL_denvmap=None), "null grad_pyramid")},
}


def test_c_abi_refusals():
    import capi_ctypes
    lib = LC.declare(capi_ctypes.load())
    RU.run_refusals(lib, LOOKUP_INTS, LOOKUP_PTRS, SIZES, NULL_BY_DEFAULT, LOOKUP_EVERY_CALL, LOOKUP_PER_CALL)
    RU.run_refusals(lib, BUILDER_INTS, BUILDER_PTRS, SIZES, (), SPEC_REFUSALS, BUILDER_PER_CALL)
    # the order the header documents is the order tested above
    order = re.sub(r"\s*\n \* ", " ", HEADER_TEXT[HEADER_TEXT.index("The order:"):])
    at = [order.index(w) for w in ('"bad rows"', "C, L,", "at least one texel", "multiples of 2^(L-1)", '"pyramid too large"', '"lod_stride must be at least 1"', "null d,",
                                   "null lod,", "null pyramid", "a null output (dmr_envmap_lod_rows,", "a null grad_out", "a null envmap", "a null grad_pyramid")]
    assert at == sorted(at)


# ---------------------------------------------------------------------------
# The case tables of the GPU tests
# ---------------------------------------------------------------------------
def test_dispatch_restated_as_the_unit_has_it():
    product = RU.dispatch_restated(LC, UNIT_TEXT, HEADER_TEXT, twice=LC.TWICE)
    assert [LC.via_lds(n) for n in LC.CHUNKS] == [False, True, True] and [LC.chunks_of(c) for c in (1, 4, 5, 8, 9, 12, 13, 16)] == [1, 1, 2, 2, 4, 4, 4, 4]
    assert "ablate_bits" not in product and "g_lod_stats" not in product and "p.dbg" not in product and "g_lod_stats" in UNIT_TEXT
    assert "k_envmap_pyramid_level<<<pyr_groups((int64_t)Hd * Wd), dim3(PYR_THREADS), 0, st>>>" in product
    assert FG._pyramid_spec("t", 64, 128, 7, 3) == LC.offsets(64, 128, 7)


def test_the_unit_waits_for_nothing_and_zeroes_nothing_by_memset():
    code = RU.waits_for_nothing([UNIT_TEXT, COORDS_TEXT, BASE_COORDS_TEXT], fill_calls=1)
    # dL_dd and dL_dlod are stored, never added: the only global atomics are the two into dL_dpyramid; the builder has none
    assert code.count("unsafeAtomicAdd(&dpyr[") == 2 and code.count("unsafeAtomicAdd(") == 2 and "atomicAdd(&dd" not in code and "atomicAdd(&dlod" not in code
    builder = code[code.index("k_envmap_pyramid_base("):code.index("struct LodParams")]
    assert "atomic" not in builder and "__shared__" not in builder and "k_envmap_pyramid_backward(" in builder


def test_tables_reach_every_instantiation():
    full = LC.every_instantiation()
    assert len(full) == 3 + 7 + 3 + 1
    tables = LC.tables()
    rest = [c for name, rows in tables.items() if name != "only" for c in rows]
    assert LC.instantiations(rest) | LC.instantiations(tables["only"], one_call=True) | LC.builder_instantiations(LC.BUILDER) == full
    # the table -- its BIG case too -- runs the full instantiation and the one without dL_dd; the single wants come from `only`
    assert LC.instantiations(LC.TABLE) == {i for i in full if i[0] in ("k_envmap_lod_rows", RU.FILL_KERNEL) or i[1] in ((True, True, True), (False, True, True))}
    assert LC.instantiations([c for c in LC.TABLE if c.N > LC.MAX_GROUPS * LC.THREADS]) >= {("k_envmap_lod_rows_backward", (True, True, True))}
    assert {c.want for c in tables["only"]} == set(LC.WANTS)
    assert {w for c in tables["only"] for w in LC.backward_calls(c.want, one_call=True)} == {("d" in w, "l" in w, "p" in w) for w in LC.WANTS}


def test_table_holds_the_shapes_that_can_go_wrong():
    t = LC.TABLE
    assert {c.N for c in t} == {0, 1, 63, 64, 65, 255, 256, 257, 1000, LC.MAX_GROUPS * LC.THREADS + 257}
    assert {c.C for c in t} == {1, 3, 4, 5, 8, 12, 16} and {(c.He, c.We, c.L) for c in t} == set(LC.PYRAMIDS)
    assert {c.layout for c in t} == set(EC.LAYOUTS) and {c.lod for c in t} == set(LC.LODS)
    assert {(He >> (L - 1), We >> (L - 1)) for He, We, L in LC.PYRAMIDS} >= {(1, 1), (1, 2), (3, 5)}   # the tops: one texel, one row, odd sizes
    for n in LC.CHUNKS:   # every chunk count below and above a workgroup's tile, with float4 reads and without
        mine = [c for c in t if LC.chunks_of(c.C) == n]
        assert any(c.N <= LC.THREADS for c in mine) and any(c.N > 2 * LC.THREADS for c in mine), n
        assert any(c.C % 4 == 0 for c in mine) and (n == 4 or any(c.C % 4 for c in mine)), n
    assert {(c[1], c[2], c[3]) for c in LC.BUILDER} >= set(LC.PYRAMIDS) and any(c[0] == 16 and c[1] == 1 << (c[3] - 1) for c in LC.BUILDER)
    for c in _all_cases():
        d, lod, env = LC.directions_of(c), LC.lod_of(c), LC.pyramid_base_of(c)
        assert d.shape == (c.N, 3) and d.dtype == np.float32 and lod.shape == (c.N,) and lod.dtype == np.float32 and env.shape == (c.He, c.We, c.C)
        if c.N == 0:
            continue
        p = LC.places64(d, lod, c.He, c.We, c.L)
        assert not p["skipped"].any() and not p["pole"].any()
        _, T = LC.offsets(c.He, c.We, c.L)
        assert p["rows"].min() >= 0 and p["rows"].max() < T and (p["w"] >= 0).all() and np.abs(p["w"].sum(0) - 1).max() <= 1e-15
        if c.lod == "uniform" and c.N >= 255 and c.L > 1:
            assert (lod < 0).any() and (lod > c.L - 1).any() and len(set(p["l"][0].tolist())) == c.L - 1     # both clamps, every pair
        if c.lod == "integer":
            assert (lod == np.round(lod)).all() and (c.N < 64 or len(set(lod.tolist())) == c.L)
        if c.lod in ("one", "pair"):
            assert len(set(p["l"][0].tolist())) == 1 and (c.lod == "pair" or len(set(lod.tolist())) == 1)
    big = [c for c in t if c.N > LC.MAX_GROUPS * LC.THREADS]
    assert len(big) == 1 and big[0].layout == "sphere" and LC.offsets(big[0].He, big[0].We, big[0].L)[1] * ((big[0].C + 3) // 4) > LC.TABLE_CELLS


def test_no_case_leaves_more_rows_out_of_the_dd_comparison_than_the_cap():
    """For the dL_dd comparison alone a row carries no upstream if it is within 1e-3 texel of a cell line of either level it uses, or
    has rho2 < 1e-4; no case may leave out more than max(5 rows, 3 % of its rows).  From the float64 model alone."""
    worst = {}
    for c in _all_cases():
        if c.N == 0:
            continue
        out = int(LC.no_dd_upstream(LC.directions_of(c), LC.lod_of(c), c.He, c.We, c.L).sum())
        assert out <= LC.exclusion_cap(c.N), (c, out)
        worst[c.N] = max(worst.get(c.N, 0), out)
    print("\nrows without upstream in the dL_dd comparison, the most per N: " + ", ".join(f"N = {n}: {k}" for n, k in sorted(worst.items())))
    # every layout on every pyramid with two or more levels, lod uniform over [-0.5, L - 0.5], at a wave and at a tile and a row
    most = {63: 0, 257: 0.0}
    for layout in EC.LAYOUTS:
        for pyr in LC.PYRAMIDS[1:]:
            for N in (63, 257):
                c = LC.case(N, 3, pyr, layout)
                out = int(LC.no_dd_upstream(LC.directions_of(c), LC.lod_of(c), c.He, c.We, c.L).sum())
                assert out <= LC.exclusion_cap(N), (c, out)
                most[N] = max(most[N], out if N == 63 else out / N)
    print(f"over the layouts and pyramids: at most {most[63]} rows at N = 63, {100 * most[257]:.2f} % at N = 257")
