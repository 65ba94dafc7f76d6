"""The environment-map unit (csrc/dmr_envmap.hip: fragments.envmap_rows_fused): which kernel instantiation a call reaches, the
launch constants the shapes of its GPU tests are built from, the case tables of tests/test_envmap_gpu.py, and the float64 numpy
model of the map from a direction to its place in the map (coords64) that both test files compare against.  No GPU code: the
GPU tests import the tables from here, and tests/test_envmap_cpu.py checks, without a GPU, that they reach every instantiation
the unit compiles and that the dispatch lines restated here are still in the unit.  In sh_cases.py's role.
"""
from collections import namedtuple

import numpy as np

from row_units import FILL_KERNEL

# ---------------------------------------------------------------------------
# The host dispatch of dmr_envmap.hip, restated.  DISPATCH_LINES holds the lines this mirrors; tests/test_envmap_cpu.py fails when
# one of them is no longer in the file exactly once: then this follows the new dispatch.
# ---------------------------------------------------------------------------
THREADS, MAX_GROUPS, MAX_C, TABLE_CELLS = 256, 1024, 16, 1024
CHUNKS = (1, 2, 4)   # the forward's instantiations: C <= 4, <= 8, <= 16
DISPATCH_LINES = [
    "constexpr int ENV_THREADS = 256, ENV_MAX_GROUPS = DMR_ENVMAP_MAX_GROUPS, ENV_MAX_C = DMR_ENVMAP_MAX_CHANNELS;",
    "constexpr bool env_via_lds(int nch) { return nch >= 2; }",
    "constexpr int ENV_TAB = 1024;",
    "with_one_of<1, 2, 4>(p.nch, [&](auto nch) {  // (the 3 instantiations of the forward: C <= 4, <= 8, <= 16 -- 3 chunks run as 4)",
    "constexpr bool L = env_via_lds(NCH);",
    "k_envmap_rows<NCH, L><<<groups, block, env_stage_bytes(NCH, L), st>>>(p, g.tiles, y);",
    "with_wanted(dL_dd != nullptr, dL_denvmap != nullptr, [&](auto wd, auto we) {  // (the 3 of the backward: an output that is not wanted is null, and its kernel has no table)",
    "constexpr bool WD = decltype(wd)::value, WE = decltype(we)::value;",
    "k_envmap_rows_backward<WD, WE><<<groups, block, 0, st>>>(p, g.tiles, grad_out, dL_dd, dL_denvmap);",
    "const RowsGrid g = rows_grid(N, ENV_THREADS, ENV_MAX_GROUPS);",
    "const dim3 groups((unsigned)g.groups), block(ENV_THREADS);",
    "const int go = rows_backward_prologue(name, N, grad_out, nullptr, dL_dd, dL_denvmap != nullptr);",
    "rows_fill_on(st, dL_denvmap, (int64_t)He * We * C, 0u);",
    "p.vec = shade_vec(C, envmap);",
    "const int64_t nch = (C + 3) / 4;",
]
TWICE = ("const RowsGrid g = rows_grid(N, ENV_THREADS, ENV_MAX_GROUPS);", "const dim3 groups((unsigned)g.groups), block(ENV_THREADS);")   # (both calls)
HEADER_LINES = ["#define DMR_ENVMAP_MAX_GROUPS 1024", "#define DMR_ENVMAP_MAX_CHANNELS 16"]
COORDS_HEADER = "dmr_envmap_coords.hpp"
COORDS_LINES = ["wrap_pair(x0, We, 1, c.ix0, c.ix1);", "wrap_pair(y0, He, 0, c.iy0, c.iy1);"]   # (... of COORDS_HEADER: the last step before the indices)


def chunks_of(C):
    """The forward's NCH for C channels: ceil(C / 4), 3 running as 4."""
    n = (C + 3) // 4
    return 4 if n == 3 else n


def via_lds(nch):
    """env_via_lds: the chunk counts whose y leaves through the LDS transpose (profiles/envmap/store_shapes.txt)."""
    return nch >= 2


# One forward + backward as the dispatch sees it.  layout: where the rows' directions lie -- "sphere": uniform; "cone": inside a
# 2-degree half-angle about one axis (many rows per texel: the merge regime); "same": all rows identical; "seam": within 0.05 rad
# of phi = +-pi; "caps": within 0.2 rad of +-z but with rho >= 0.02; "shuffled": a raster of a 40-degree field, randomly permuted
# (neighbouring lanes share no texel).  Lengths in [0.5, 3].  want: which gradients the call asks for ("de", "d", "e").
LAYOUTS = ("sphere", "cone", "same", "seam", "caps", "shuffled")
MAPS = ((1, 1), (1, 5), (5, 1), (4, 8), (7, 13), (16, 32), (64, 128))
Case = namedtuple("Case", "N C He We layout want")


def case(N, C, He, We, layout="sphere", want="de"):
    assert N >= 0 and 1 <= C <= MAX_C and (He, We) in MAPS and layout in LAYOUTS and want in ("de", "d", "e")
    return Case(N, C, He, We, layout, want)


def instantiations(cases):
    """The set of (kernel, template arguments) the calls `cases` run (N = 0 launches only the kernel that zeroes dL_denvmap)."""
    out = set()
    for c in cases:
        if c.N > 0:
            out.add(("k_envmap_rows", (chunks_of(c.C), via_lds(chunks_of(c.C)))))
            out.add(("k_envmap_rows_backward", ("d" in c.want, "e" in c.want)))
        if "e" in c.want:
            out.add((FILL_KERNEL, ()))
    return out


def every_instantiation():
    full = {("k_envmap_rows", (n, via_lds(n))) for n in CHUNKS}
    full |= {("k_envmap_rows_backward", w) for w in ((True, True), (True, False), (False, True))}
    return full | {(FILL_KERNEL, ())}


BIG = MAX_GROUPS * THREADS + 257   # one workgroup tile more than the capped grid holds, and an odd tail


def _table():
    t = []
    # N around a wave and a workgroup's tile; every C (float4 reads at 4, 8, 16; 3 chunks at 9..12 are C = 5's path with one more);
    # every map; every layout
    t += [case(0, 3, 4, 8), case(1, 3, 1, 1, "same"), case(1, 16, 7, 13), case(63, 1, 1, 5, "seam"), case(63, 5, 16, 32, "cone"),
          case(64, 4, 5, 1, "caps"), case(64, 8, 4, 8, "shuffled"), case(65, 3, 7, 13, "seam"), case(65, 16, 16, 32, "same"),
          case(255, 1, 64, 128, "cone"), case(255, 8, 7, 13, "caps"), case(256, 3, 16, 32, "sphere"), case(256, 5, 1, 1, "sphere"),
          case(257, 4, 64, 128, "shuffled"), case(257, 16, 1, 5, "sphere"), case(257, 3, 5, 1, "sphere")]
    # several tiles: the merge regime and the table's refusals on each chunk count
    t += [case(1000, 3, 64, 128, "sphere"), case(1000, 3, 16, 32, "cone"), case(1000, 4, 4, 8, "same"), case(1000, 8, 64, 128, "shuffled"),
          case(1000, 16, 64, 128, "sphere"), case(1000, 5, 7, 13, "caps"), case(1000, 1, 16, 32, "seam"), case(1000, 16, 16, 32, "cone"),
          case(1000, 12, 7, 13, "sphere"), case(1000, 3, 64, 128, "caps")]
    # a workgroup takes a second tile; the table fills past its half (sphere on the largest map)
    t += [case(BIG, 3, 64, 128, "sphere"), case(BIG, 8, 16, 32, "cone")]
    return t


TABLE = _table()
ONLY = [case(130, 3, 7, 13, "sphere"), case(200, 8, 16, 32, "cone"), case(270, 16, 64, 128, "shuffled")]   # each single gradient alone
MISALIGNED = [case(257, 4, 7, 13, "sphere"), case(130, 8, 16, 32, "cone"), case(65, 16, 4, 8, "sphere"), case(100, 3, 7, 13, "seam")]
N_ROWS = case(300, 3, 16, 32, "sphere")     # the counts 0, below N, N, above N, negative
GRAPH = case(700, 3, 16, 32, "sphere")
SPECIAL = (4, 7, 13)                        # C, He, We of the special rows


def tables():
    """Every table above as the calls it makes: {name: [Case]}."""
    only = [c._replace(want=w) for c in ONLY for w in ("de", "d", "e")]
    return {"table": TABLE, "only": only, "misaligned": MISALIGNED, "n_rows": [N_ROWS], "graph": [GRAPH]}


def _unit(rng, n):
    d = rng.standard_normal((n, 3))
    return d / np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-3)


def _sph(theta, phi):
    return np.stack([np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi), np.cos(theta)], -1)


def directions_of(c, seed=0):
    """d float32 [N,3] of a case as numpy: the layout's unit vectors times a length in [0.5, 3]."""
    rng = np.random.default_rng(3000 * seed + 7 * c.N + 13 * c.C + 17 * c.He + c.We + LAYOUTS.index(c.layout))
    n = c.N
    if c.layout == "sphere":
        u = _unit(rng, n)
    elif c.layout in ("cone", "shuffled"):
        half = np.radians(2.0 if c.layout == "cone" else 20.0)
        axis = np.array([0.55, -0.35, 0.45])
        axis /= np.linalg.norm(axis)
        e1 = np.cross(axis, [0.0, 0.0, 1.0])
        e1 /= np.linalg.norm(e1)
        e2 = np.cross(axis, e1)
        if c.layout == "cone":
            r, a = np.tan(half) * np.sqrt(rng.random(n)), 2 * np.pi * rng.random(n)
            px, py = r * np.cos(a), r * np.sin(a)
        else:   # a raster, row-major, then permuted
            side = int(np.ceil(np.sqrt(max(n, 1))))
            gy, gx = np.divmod(np.arange(n), side)
            px, py = ((gx + 0.5) / side * 2 - 1) * np.tan(half), ((gy + 0.5) / side * 2 - 1) * np.tan(half)
            perm = rng.permutation(n)
            px, py = px[perm], py[perm]
        u = axis + px[:, None] * e1 + py[:, None] * e2
        u /= np.linalg.norm(u, axis=1, keepdims=True)
    elif c.layout == "same":
        u = np.repeat(_sph(np.array([1.1 + 0.37 * rng.random()]), np.array([0.9 + 0.41 * rng.random()])), n, 0)
    elif c.layout == "seam":
        sign = np.where(rng.random(n) < 0.5, -1.0, 1.0)
        u = _sph(0.3 + (np.pi - 0.6) * rng.random(n), sign * (np.pi - 0.05 * rng.random(n)))
    else:   # "caps": sin(0.0201) > 0.02
        theta = 0.0201 + (0.2 - 0.0201) * rng.random(n)
        u = _sph(np.where(rng.random(n) < 0.5, theta, np.pi - theta), 2 * np.pi * rng.random(n) - np.pi)
    return (u * rng.uniform(0.5, 3.0, (n, 1))).astype(np.float32)


def envmap_of(c, seed=0):
    """envmap float32 [He,We,C] of a case: N(0, 1)."""
    rng = np.random.default_rng(4000 * seed + 13 * c.C + 17 * c.He + c.We)
    return rng.standard_normal((c.He, c.We, c.C)).astype(np.float32)


# ---------------------------------------------------------------------------
# The header's encoding in float64 numpy, written from include/dmesh_renderer_amd_envmap.h, not from fragments.py
# ---------------------------------------------------------------------------
def coords64(d, He, We, dtype_of_n=np.float32):
    """d [N,3] -> dict(skipped, pole, rho2, x, y, fx, fy, ix0, ix1, iy0, iy1) in float64; n (what decides `skipped`) in
    dtype_of_n, as the kernels and the float32 model form it."""
    d = np.asarray(d)
    with np.errstate(all="ignore"):
        dn = d.astype(dtype_of_n)
        n = np.sqrt((dn * dn).sum(1, dtype=dtype_of_n))
        skipped = ~(np.isfinite(n) & (n >= dtype_of_n(1e-8)))
        d64 = np.where(skipped[:, None], np.array([1.0, 0.0, 0.0]), d.astype(np.float64))
        u = d64 / np.sqrt((d64 * d64).sum(1, keepdims=True))
        rho2 = u[:, 0] ** 2 + u[:, 1] ** 2
        pole = (rho2 < 1e-12) & ~skipped
        theta = np.arccos(np.clip(u[:, 2], -1, 1))
        phi = np.where(pole, 0.0, np.arctan2(u[:, 1], u[:, 0]))
        x = (phi / (2 * np.pi) + 0.5) * We - 0.5
        y = theta / np.pi * He - 0.5
        x0, y0 = np.floor(x), np.floor(y)
        ix0, ix1 = np.mod(x0, We).astype(np.int64), np.mod(x0 + 1, We).astype(np.int64)
        iy0, iy1 = np.clip(y0, 0, He - 1).astype(np.int64), np.clip(y0 + 1, 0, He - 1).astype(np.int64)
    return dict(skipped=skipped, pole=pole, rho2=rho2, x=x, y=y, fx=x - x0, fy=y - y0, ix0=ix0, ix1=ix1, iy0=iy0, iy1=iy1)


def no_dd_upstream(d, He, We):
    """bool [N]: the rows that carry no upstream in the dL_dd comparison -- within 1e-3 texel of a cell line (there float32 and
    float64 may sit in different cells, and the derivative jumps) or with rho2 < 1e-4 (acos' derivative)."""
    c = coords64(d, He, We)
    near = lambda f: np.minimum(f, 1 - f) < 1e-3
    return (near(c["fx"]) | near(c["fy"]) | (c["rho2"] < 1e-4)) & ~c["skipped"]
