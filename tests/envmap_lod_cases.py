"""The pyramid unit (csrc/dmr_envmap_lod.hip: fragments.envmap_pyramid_fused, envmap_lod_rows_fused): which kernel instantiation a
call reaches, the launch constants the shapes of its GPU tests are built from, the case tables of tests/test_envmap_lod_gpu.py,
the float64 numpy model of the level choice and of the placement per level (levels64, places64) written from
include/dmesh_renderer_amd_envmap_lod.h, not from fragments.py, and the unit's own ctypes signatures.  No GPU code: the GPU tests
import the tables from here, and tests/test_envmap_lod_cpu.py checks, without a GPU, that they reach every instantiation the
unit compiles, that the dispatch lines restated here are still in the unit, and that no case leaves more rows out of its dL_dd
comparison than the cap allows.  In envmap_cases.py's role, on its layouts and its coords64.
"""
import ctypes as C
from collections import namedtuple

import numpy as np

import envmap_cases as EC
from row_units import FILL_KERNEL

# ---------------------------------------------------------------------------
# The host dispatch of dmr_envmap_lod.hip, restated.  DISPATCH_LINES holds the lines this mirrors; tests/test_envmap_lod_cpu.py
# fails when one of them is no longer in the file exactly once: then this follows the new dispatch.
# ---------------------------------------------------------------------------
THREADS, MAX_GROUPS, MAX_C, MAX_L, TABLE_CELLS = 256, 1024, 16, 12, 1024
CHUNKS = (1, 2, 4)   # the forward's instantiations: C <= 4, <= 8, <= 16
WANTS = ("d", "l", "dl", "p", "dp", "lp", "dlp")   # the backward's: d = dL_dd, l = dL_dlod, p = dL_dpyramid
BUILDER_KERNELS = ("k_envmap_pyramid_base", "k_envmap_pyramid_level", "k_envmap_pyramid_backward")
DISPATCH_LINES = [
    "constexpr int LOD_THREADS = 256, LOD_MAX_GROUPS = DMR_ENVMAP_LOD_MAX_GROUPS, LOD_MAX_C = DMR_ENVMAP_LOD_MAX_CHANNELS, LOD_MAX_L = DMR_ENVMAP_LOD_MAX_LEVELS;",
    "constexpr bool lod_via_lds(int nch) { return nch >= 2; }",
    "constexpr int LOD_TAB = 1024;",
    "with_one_of<1, 2, 4>(p.nch, [&](auto nch) {  // (the 3 instantiations of the forward: C <= 4, <= 8, <= 16 -- 3 chunks run as 4)",
    "constexpr bool S = lod_via_lds(NCH);",
    "k_envmap_lod_rows<NCH, S><<<groups, block, lod_stage_bytes(NCH, S), st>>>(p, g.tiles, y);",
    "with_one_of<1, 2, 3, 4, 5, 6, 7>((d ? 1 : 0) | (l ? 2 : 0) | (pyr ? 4 : 0), [&](auto m) {",
    "f(std::bool_constant<(M & 1) != 0>(), std::bool_constant<(M & 2) != 0>(), std::bool_constant<(M & 4) != 0>());",
    "constexpr bool WD = decltype(wd)::value, WL = decltype(wl)::value, WP = decltype(wp)::value;",
    "k_envmap_lod_rows_backward<WD, WL, WP><<<groups, block, 0, st>>>(p, g.tiles, grad_out, dL_dd, dL_dlod, dL_dpyramid);",
    "const RowsGrid g = rows_grid(N, LOD_THREADS, LOD_MAX_GROUPS);",
    "const dim3 groups((unsigned)g.groups), block(LOD_THREADS);",
    "if (N == 0) dL_dlod = nullptr;  // (no row to write)",
    "const int go = rows_backward_prologue(name, N, grad_out, nullptr, dL_dd, dL_dlod != nullptr || dL_dpyramid != nullptr);",
    "rows_fill_on(st, dL_dpyramid, T * C, 0u);",
    "p.vec = shade_vec(C, pyramid);",
    "p.nch = (C + 3) / 4;",
    "k_envmap_pyramid_base<<<pyr_groups(n0), dim3(PYR_THREADS), 0, st>>>(envmap, pyramid, n0);",
    "for (int l = 1; l < L; l++) {  // (level l from level l - 1, stream-ordered)",
    "k_envmap_pyramid_backward<<<pyr_groups((int64_t)He * We), dim3(PYR_THREADS), 0, st>>>(grad_pyramid, dL_denvmap, He, We, C, L);",
]
TWICE = ("const RowsGrid g = rows_grid(N, LOD_THREADS, LOD_MAX_GROUPS);", "const dim3 groups((unsigned)g.groups), block(LOD_THREADS);")   # (both calls)
HEADER_LINES = ["#define DMR_ENVMAP_LOD_MAX_GROUPS 1024", "#define DMR_ENVMAP_LOD_MAX_CHANNELS 16", "#define DMR_ENVMAP_LOD_MAX_LEVELS 12"]
COORDS_HEADER = "dmr_envmap_lod_coords.hpp"
# (... of COORDS_HEADER: the last steps before the indices and the levels)
COORDS_LINES = ["wrap_pair(x0, We, 1, c.ix0, c.ix1);", "wrap_pair(y0, He, 0, c.iy0, c.iy1);", "v.l0 = l0 < last ? l0 : last;", "v.l1 = l1 < last ? l1 : last;"]

# The unit's C calls: name -> (leading ints, pointers with the trailing stream), row_units.SIGNATURES' form
SIGNATURES = {"dmr_envmap_pyramid": (4, 3), "dmr_envmap_pyramid_backward": (4, 3), "dmr_envmap_lod_rows": (6, 6), "dmr_envmap_lod_rows_backward": (6, 9)}


def declare(lib, names=tuple(SIGNATURES)):
    """row_units.declare for this unit's calls -> lib."""
    for name in names:
        ints, pointers = SIGNATURES[name]
        f = getattr(lib, name)
        f.restype, f.argtypes = C.c_int, [C.c_int] * ints + [C.c_void_p] * pointers
    lib.dmr_last_error.restype = C.c_char_p
    return lib


chunks_of, via_lds = EC.chunks_of, EC.via_lds   # (the forward's ladder and store shapes are dmr_envmap.hip's)


# ---------------------------------------------------------------------------
# The layout, restated from the header
# ---------------------------------------------------------------------------
def offsets(He, We, L):
    """([off_0 .. off_{L-1}], T): level l is the [He >> l, We >> l, C] block that starts at row off_l."""
    assert 1 <= L <= MAX_L and He >= 1 and We >= 1 and He % (1 << (L - 1)) == 0 and We % (1 << (L - 1)) == 0
    offs, T = [], 0
    for l in range(L):
        offs.append(T)
        T += (He >> l) * (We >> l)
    return offs, T


# Pyramids: 1 x 1 with one level; a top level of one row; a top of 1 x 2; sizes that are no powers of two; two larger ones
PYRAMIDS = ((1, 1, 1), (2, 4, 2), (4, 8, 3), (12, 20, 3), (16, 32, 5), (64, 128, 7))
# lod: "uniform" over [-0.5, L - 0.5] (both clamps); "one": all rows one value inside a pair; "integer": exact integers 0 .. L-1;
# "pair": all rows inside one level pair
LODS = ("uniform", "one", "integer", "pair")
Case = namedtuple("Case", "N C He We L layout lod want seed")


def case(N, C, pyr, layout="sphere", lod="uniform", want="dlp", seed=0):
    assert N >= 0 and 1 <= C <= MAX_C and pyr in PYRAMIDS and layout in EC.LAYOUTS and lod in LODS and want in WANTS
    return Case(N, C, *pyr, layout, lod, want, seed)


def backward_calls(want, one_call=False):
    """The backward calls a GPU test makes for a case that wants `want`, each as its (WD, WL, WP).  one_call: the single call of
    test_only_what_is_asked.  Else test_envmap_lod_gpu._run's two: dL_dd comes from the upstream without the rows near a cell line, in
    one call for everything wanted (the full instantiation on every table case); dL_dlod and dL_dpyramid come from the full upstream,
    in a second call without dL_dd."""
    d, l, p = ("d" in want, "l" in want, "p" in want)
    if one_call:
        return [(d, l, p)]
    return ([(d, l, p)] if d else []) + ([(False, l, p)] if l or p else [])


def instantiations(cases, one_call=False):
    """The set of (kernel, template arguments) the lookups `cases` run (N = 0 launches only the kernel that zeroes dL_dpyramid)."""
    out = set()
    for c in cases:
        if c.N > 0:
            out.add(("k_envmap_lod_rows", (chunks_of(c.C), via_lds(chunks_of(c.C)))))
            out |= {("k_envmap_lod_rows_backward", w) for w in backward_calls(c.want, one_call)}
        if "p" in c.want:
            out.add((FILL_KERNEL, ()))
    return out


def builder_instantiations(specs):
    """... and the builder's kernels for the pyramids `specs` ((C, He, We, L)): the level kernel runs where there is a second level."""
    out = set()
    for _, _, _, L in specs:
        out |= {("k_envmap_pyramid_base", ()), ("k_envmap_pyramid_backward", ())} | ({("k_envmap_pyramid_level", ())} if L > 1 else set())
    return out


def every_instantiation():
    full = {("k_envmap_lod_rows", (n, via_lds(n))) for n in CHUNKS}
    full |= {("k_envmap_lod_rows_backward", ("d" in w, "l" in w, "p" in w)) for w in WANTS}
    return full | {(k, ()) for k in BUILDER_KERNELS} | {(FILL_KERNEL, ())}


BIG = MAX_GROUPS * THREADS + 257   # one workgroup tile more than the capped grid holds, and an odd tail


def _table():
    t = []
    # N around a wave and a workgroup's tile; every C; every pyramid; every layout; every kind of lod
    t += [case(0, 3, (4, 8, 3)), case(1, 3, (1, 1, 1), "same", "one"), case(1, 16, (12, 20, 3)), case(63, 1, (2, 4, 2), "seam"),
          case(63, 5, (16, 32, 5), "cone", "pair"), case(64, 4, (4, 8, 3), "caps", "integer"), case(64, 8, (12, 20, 3), "shuffled"),
          case(65, 3, (12, 20, 3), "seam", "one"), case(65, 16, (16, 32, 5), "same"), case(255, 1, (64, 128, 7), "cone"),
          case(255, 8, (2, 4, 2), "caps", "pair"), case(256, 3, (16, 32, 5), "sphere", "integer"), case(256, 5, (1, 1, 1), "sphere"),
          case(257, 4, (64, 128, 7), "shuffled"), case(257, 16, (2, 4, 2), "sphere"), case(257, 12, (4, 8, 3), "sphere", "one")]
    # several tiles: the merge regime and the table's refusals on each chunk count
    t += [case(1000, 3, (64, 128, 7), "sphere"), case(1000, 3, (16, 32, 5), "cone"), case(1000, 4, (4, 8, 3), "same", "integer"),
          case(1000, 8, (64, 128, 7), "shuffled", "pair"), case(1000, 16, (64, 128, 7), "sphere"), case(1000, 5, (12, 20, 3), "caps"),
          case(1000, 1, (16, 32, 5), "seam", "one"), case(1000, 12, (12, 20, 3), "sphere")]
    # a workgroup takes a second tile; the table fills past its half (sphere on the largest pyramid)
    t += [case(BIG, 3, (64, 128, 7), "sphere")]
    return t


TABLE = _table()
ONLY = [case(130, 3, (12, 20, 3), "sphere"), case(270, 16, (16, 32, 5), "cone")]   # each of the seven want-combinations
MISALIGNED = [case(257, 4, (12, 20, 3), "sphere"), case(130, 8, (16, 32, 5), "cone"), case(65, 16, (4, 8, 3), "sphere"), case(100, 3, (2, 4, 2), "seam")]
STRIDED = [case(300, 3, (16, 32, 5), "sphere"), case(65, 8, (4, 8, 3), "cone")]
N_ROWS = case(300, 3, (16, 32, 5), "sphere")     # the counts 0, below N, N, above N, negative
GRAPH = case(700, 3, (16, 32, 5), "sphere")
AGAINST_ENVMAP = [case(257, 3, (16, 32, 5), "sphere"), case(130, 8, (1, 1, 1), "sphere"), case(300, 16, (12, 20, 3), "seam")]   # at lod <= 0 (and L == 1)
SPECIAL = (4, 12, 20, 3)                         # C, He, We, L of the special rows
# the builder, (C, He, We, L): every pyramid shape above, C = 16 on 8 x 8 with as many levels as the rows allow (the top is one
# texel), and a single level
BUILDER = [(3, 1, 1, 1), (1, 2, 4, 2), (4, 4, 8, 3), (5, 12, 20, 3), (8, 16, 32, 5), (3, 64, 128, 7), (16, 8, 8, 4), (12, 12, 20, 1)]


def tables():
    """Every table of lookups above as the calls it makes: {name: [Case]}."""
    only = [c._replace(want=w) for c in ONLY for w in WANTS]
    return {"table": TABLE, "only": only, "misaligned": MISALIGNED, "strided": STRIDED, "n_rows": [N_ROWS], "graph": [GRAPH], "against": AGAINST_ENVMAP}


def directions_of(c, seed=None):
    """d float32 [N,3] of a case: envmap_cases' layout on the base map's size."""
    return EC.directions_of(c, c.seed if seed is None else seed)


def lod_of(c, seed=None):
    """lod float32 [N] of a case, by its kind."""
    seed = c.seed if seed is None else seed
    rng = np.random.default_rng(5000 * seed + 7 * c.N + 13 * c.C + 17 * c.He + c.L + LODS.index(c.lod))
    if c.lod == "uniform":
        lod = rng.uniform(-0.5, c.L - 0.5, c.N)
    elif c.lod == "one":
        lod = np.full(c.N, max(c.L - 2, 0) + 0.37)
    elif c.lod == "integer":
        lod = rng.integers(0, c.L, c.N).astype(np.float64)
    else:
        lod = max(c.L - 2, 0) + rng.uniform(0.02, 0.98, c.N)
    return lod.astype(np.float32)


def pyramid_base_of(c, seed=None):
    """the base map float32 [He,We,C] of a case: N(0, 1)."""
    seed = c.seed if seed is None else seed
    rng = np.random.default_rng(4000 * seed + 13 * c.C + 17 * c.He + c.We + c.L)
    return rng.standard_normal((c.He, c.We, c.C)).astype(np.float32)


# ---------------------------------------------------------------------------
# The header's level choice and placement in float64 numpy, written from include/dmesh_renderer_amd_envmap_lod.h
# ---------------------------------------------------------------------------
def levels64(lod, L):
    """lod [N] -> (l0, l1 int64, f float64, inside bool): lam = lod clamped into [0, L-1] (NaN: 0), l0 = min(floor(lam), L-2),
    l1 = l0 + 1, f = lam - l0; L == 1: l0 = l1 = 0, f = 0, inside false."""
    lod = np.asarray(lod, dtype=np.float64)
    with np.errstate(all="ignore"):
        lam = np.where(lod >= 0, np.where(lod <= L - 1, lod, float(L - 1)), 0.0)
        inside = (lod > 0) & (lod < L - 1)
    if L == 1:
        z = np.zeros(lod.shape, dtype=np.int64)
        return z, z.copy(), np.zeros(lod.shape), inside
    l0 = np.minimum(np.floor(lam), L - 2).astype(np.int64)
    return l0, l0 + 1, lam - l0, inside


def places64(d, lod, He, We, L):
    """Per row its two levels' places: dict(l, w, He, We, fx, fy, ix0, ix1, iy0, iy1, rows), each [2,N] (k = 0: l0 with weight 1-f,
    k = 1: l1 with weight f; rows: the texel's row of the pyramid, [2,4,N] in the order 00, 01, 10, 11) and skipped, pole, inside [N]."""
    d = np.asarray(d)
    N = d.shape[0]
    l0, l1, f, inside = levels64(lod, L)
    offs, _ = offsets(He, We, L)
    base = EC.coords64(d, He, We)
    out = dict(l=np.stack([l0, l1]), w=np.stack([1 - f, f]), skipped=base["skipped"], pole=base["pole"], inside=inside, rho2=base["rho2"])
    for k in ("He", "We", "ix0", "ix1", "iy0", "iy1"):
        out[k] = np.zeros((2, N), dtype=np.int64)
    out["fx"], out["fy"], out["rows"] = np.zeros((2, N)), np.zeros((2, N)), np.zeros((2, 4, N), dtype=np.int64)
    for l in range(L):
        c = EC.coords64(d, He >> l, We >> l)
        for k in range(2):
            m = out["l"][k] == l
            out["He"][k, m], out["We"][k, m] = He >> l, We >> l
            for key in ("fx", "fy", "ix0", "ix1", "iy0", "iy1"):
                out[key][k, m] = c[key][m]
            for i, (iy, ix) in enumerate((("iy0", "ix0"), ("iy0", "ix1"), ("iy1", "ix0"), ("iy1", "ix1"))):
                out["rows"][k, i, m] = offs[l] + c[iy][m] * (We >> l) + c[ix][m]
    return out


def may_touch(d, lod, He, We, L):
    """bool [T]: the rows of the pyramid a float32 lookup of these rows may read or add into -- per level of nonzero weight the
    4 x 4 texels around the float64 cell (columns repeat, rows clamp): a superset of the call's 2 x 2 as long as float32 puts a row
    within one cell of where float64 puts it, however close to a cell line the row lies.  Every other row of dL_dpyramid is an
    exact 0."""
    d = np.asarray(d)
    l0, l1, f, _ = levels64(lod, L)
    offs, T = offsets(He, We, L)
    out = np.zeros(T, dtype=bool)
    for l in range(L):
        used = ((l0 == l) & (1 - f != 0)) | ((l1 == l) & (f != 0))
        c = EC.coords64(d[used], He >> l, We >> l)
        x0, y0 = np.floor(c["x"][~c["skipped"]]).astype(np.int64), np.floor(c["y"][~c["skipped"]]).astype(np.int64)
        for dy in (-1, 0, 1, 2):
            for dx in (-1, 0, 1, 2):
                out[offs[l] + np.clip(y0 + dy, 0, (He >> l) - 1) * (We >> l) + np.mod(x0 + dx, We >> l)] = True
    return out


def no_dd_upstream(d, lod, He, We, L):
    """bool [N]: the rows that carry no upstream in the dL_dd comparison -- envmap_cases.no_dd_upstream applied per used level
    (a level whose weight is not 0): within 1e-3 texel of a cell line of either level the row uses, or rho2 < 1e-4."""
    l0, l1, f, _ = levels64(lod, L)
    quiet = np.zeros(np.asarray(d).shape[0], dtype=bool)
    for l in range(L):
        used = ((l0 == l) & (1 - f != 0)) | ((l1 == l) & (f != 0))
        quiet |= EC.no_dd_upstream(d, He >> l, We >> l) & used
    return quiet


def exclusion_cap(N):
    """The most rows a case may leave out of its dL_dd comparison: max(5 rows, 3 % of its rows)."""
    return max(5, int(0.03 * N))
