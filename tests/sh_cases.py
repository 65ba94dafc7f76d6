"""The spherical-harmonics unit (csrc/dmr_sh.hip: fragments.sh_rows_fused, packed_row_views_fused): which kernel instantiation a
call reaches, the launch constants the shapes of its GPU tests are built from, and the case tables of tests/test_sh_gpu.py.  No
GPU code: the GPU tests import the tables from here, and tests/test_sh_cpu.py checks, without a GPU, that they reach every
instantiation the unit compiles and that the dispatch lines restated here are still in the unit.  In hashgrid_cases.py's role.
"""
from collections import namedtuple

import numpy as np

from row_units import FILL_KERNEL

# ---------------------------------------------------------------------------
# The host dispatch of dmr_sh.hip, restated.  DISPATCH_LINES holds the lines this mirrors; tests/test_sh_cpu.py fails when one of
# them is no longer in the file exactly once: then this follows the new dispatch.  What the row units take from the shared
# csrc/dmr_rows_common.* is restated once, in tests/row_units.py (COMMON_DISPATCH_LINES, FILL_KERNEL).
# ---------------------------------------------------------------------------
DEGREES = (1, 2, 3, 4)
THREADS, MAX_GROUPS, MAX_VIEWS = 256, 1024, 1024
DISPATCH_LINES = [
    "constexpr int SH_THREADS = 256, SH_MAX_GROUPS = DMR_SH_MAX_GROUPS, SH_MAX_VIEWS = DMR_SH_MAX_VIEWS;",
    "constexpr bool sh_via_lds(int degree) { return degree >= 3; }",
    "with_one_of<1, 2, 3, 4>(degree, [&](auto deg) {  // (the 4 instantiations of the forward)",
    "with_one_of<1, 2, 3, 4>(degree, [&](auto deg) {  // (... the 12 of the backward)",
    "constexpr bool sh_loads_via_lds(int) { return false; }",
    "constexpr bool L = sh_via_lds(D);",
    "constexpr bool L = sh_loads_via_lds(D);",
    "k_sh_rows<D, L><<<groups, block, sh_stage_bytes(D, L), st>>>(p, g.tiles, y);",
    "with_wanted(dL_dx != nullptr, dL_dorigin != nullptr, [&](auto wx, auto wo) {  // (an output that is not wanted is null, and its kernel has no table)",
    "constexpr bool WX = decltype(wx)::value, WO = decltype(wo)::value;",
    "const size_t table = WO ? tab : 0;",
    "k_sh_rows_backward<D, WX, WO, L><<<groups, block, table + sh_stage_bytes(D, L), st>>>(p, g.tiles, (int)table, grad_out, dL_dx, dL_dorigin);",
    "const RowsGrid g = rows_grid(N, SH_THREADS, SH_MAX_GROUPS);",
    "const dim3 groups((unsigned)g.groups), block(SH_THREADS);",
    'const int go = rows_backward_prologue(name, N, grad_out, dL_dorigin && !origin ? "dL_dorigin without origin" : nullptr, dL_dx, dL_dorigin != nullptr);',
    "rows_fill_on(st, dL_dorigin, (int64_t)3 * B, 0u);",
    "rows_fill_on(st, view_out, N, 0xffffffffu);",
    "if (N == 0 || !slots) return 0;",
]
TWICE = ("const RowsGrid g = rows_grid(N, SH_THREADS, SH_MAX_GROUPS);", "const dim3 groups((unsigned)g.groups), block(SH_THREADS);")   # (both calls)
HEADER_LINES = ["#define DMR_SH_MAX_GROUPS 1024", "#define DMR_SH_MAX_VIEWS 1024", "#define DMR_SH_MAX_DEGREE 4"]


def via_lds(degree):
    """sh_via_lds: the degrees whose y leaves through the LDS transpose."""
    return degree >= 3


def loads_via_lds(degree):
    """sh_loads_via_lds: the degrees whose upstream arrives through the LDS transpose -- none (profiles/sh/store_shapes.txt)."""
    return False


# One forward + backward as the dispatch sees it.  layout: how the rows' views follow each other -- "one": every row view B - 1;
# "major": view-major blocks of uneven length (what pack_slots gives); "mixed": the view changes every 7 rows (inside every
# wave: the per-lane adds); "wave": exactly at every wave's edge; "group": exactly at every workgroup's edge; "shuffled": a
# random permutation of "major"; "holes": "major" with -1 and B (and beyond) scattered over a sixth of the rows.
# form: "views" (origin [B,3] and row_view), "single" (origin [1,3], no row_view), "dirs" (origin=None: x holds w).
# want: which gradients the call asks for ("xo", "x", "o").
LAYOUTS = ("one", "major", "mixed", "wave", "group", "shuffled", "holes")
Case = namedtuple("Case", "N degree B layout form want")


def case(N, degree, B, layout="major", form="views", want=None):
    want = want or ("x" if form == "dirs" else "xo")
    assert N >= 0 and degree in DEGREES and 1 <= B <= MAX_VIEWS and layout in LAYOUTS and form in ("views", "single", "dirs") and want in ("xo", "x", "o")
    assert form == "views" or (B == 1 and layout == "one")
    assert form != "dirs" or want == "x"
    return Case(N, degree, B, layout, form, want)


def instantiations(cases):
    """The set of (kernel, template arguments) the calls `cases` run (N = 0 launches only the kernel that zeroes dL_dorigin)."""
    out = set()
    for c in cases:
        if c.N > 0:
            out.add(("k_sh_rows", (c.degree, via_lds(c.degree))))
            out.add(("k_sh_rows_backward", (c.degree, "x" in c.want, "o" in c.want, loads_via_lds(c.degree))))
        if "o" in c.want:
            out.add((FILL_KERNEL, ()))
    return out


def every_instantiation():
    full = {("k_sh_rows", (d, via_lds(d))) for d in DEGREES}
    full |= {("k_sh_rows_backward", (d, wx, wo, loads_via_lds(d))) for d in DEGREES for wx, wo in ((True, True), (True, False), (False, True))}
    return full | {(FILL_KERNEL, ()), ("k_sh_row_views", ())}


def _table():
    t = []
    # N around a wave and a workgroup's tile, every degree (both store shapes), B in {1, 2, 5}, every layout
    t += [case(0, 4, 2), case(1, 4, 1, "one", "single"), case(1, 1, 2, "one"), case(63, 1, 2, "mixed"), case(63, 3, 5, "shuffled"),
          case(64, 2, 5, "mixed"), case(64, 4, 2, "wave"), case(65, 3, 2, "wave"), case(65, 2, 1, "one", "dirs"),
          case(255, 4, 5, "shuffled"), case(255, 1, 1, "one", "single"), case(256, 3, 5, "holes"), case(256, 4, 2, "group"),
          case(257, 4, 2, "wave"), case(257, 3, 1, "one", "dirs"), case(257, 2, 5, "holes"), case(257, 1, 5, "major")]
    # several tiles: every degree on the layouts that take the wave's sum ("one", "major", "wave", "group") and the per-lane adds
    t += [case(1000, 1, 5, "group"), case(1000, 2, 2, "major"), case(1000, 3, 5, "major"), case(1000, 4, 5, "major"),
          case(777, 3, 2, "mixed"), case(777, 4, 5, "mixed"), case(900, 4, 5, "holes"), case(900, 3, 5, "group"),
          case(700, 4, 1, "one", "dirs"), case(700, 4, 1, "one", "single"), case(1000, 2, 5, "shuffled"), case(1000, 4, 2, "one")]
    # one workgroup tile more than the capped grid holds: a workgroup takes a second tile
    t += [case(MAX_GROUPS * THREADS + 1, 4, 2, "major"), case(MAX_GROUPS * THREADS + 257, 3, 5, "group")]
    return t


TABLE = _table()
ONLY = [case(130 + 70 * i, d, 2, ("mixed", "major")[i % 2]) for i, d in enumerate(DEGREES)]   # each single gradient alone
MISALIGNED = [case(257, 4, 2, "major"), case(130, 3, 5, "mixed"), case(65, 2, 2, "major"), case(100, 1, 1, "one", "single")]   # x and y one float off a 16-byte boundary
N_ROWS = case(300, 4, 2, "major")     # the counts 0, below N, N, above N, negative
GRAPH = case(700, 4, 2, "major")
CHAIN = dict(n_levels=8, features=4, log2_table_size=12, base_resolution=4, per_level_scale=1.5, degree=4, hidden=64)   # HashGrid 32 + ViewSH 16 -> RowMLP(48, 64, 3)
# the packed unit's shapes for packed_row_views_fused: (B, K, H, W, the share of used slots); capacities come per case
VIEW_SHAPES = [(1, 1, 1, 1, 1.0), (1, 1, 1, 1, 0.0), (2, 5, 17, 33, 0.4), (3, 1, 4, 64, 1.0), (2, 32, 9, 70, 0.3), (1, 5, 258 * 4, 64, 0.5),
               (2, 5, 17, 33, 0.0), (5, 1, 3, 130, 0.7)]


def tables():
    """Every table above as the calls it makes: {name: [Case]}."""
    only = [c._replace(want=w) for c in ONLY for w in ("xo", "x", "o")]
    return {"table": TABLE, "only": only, "misaligned": MISALIGNED, "n_rows": [N_ROWS], "graph": [GRAPH],
            "chain": [case(1, CHAIN["degree"], 2, "major")]}


def views_of(c, seed=0):
    """row_view int32 [N] of a case as numpy (for every form: "single" and "dirs" do not pass it on)."""
    rng = np.random.default_rng(1000 * seed + 7 * c.N + 13 * c.degree + c.B)
    r = np.arange(c.N)
    if c.layout == "one":
        v = np.full(c.N, c.B - 1)
    elif c.layout == "mixed":
        v = (r // 7) % c.B
    elif c.layout == "wave":
        v = (r // 64) % c.B
    elif c.layout == "group":
        v = (r // THREADS) % c.B
    else:
        cuts = np.sort(rng.integers(0, c.N + 1, c.B - 1)) if c.B > 1 else np.zeros(0, dtype=np.int64)
        v = np.searchsorted(cuts, r, side="right")
        if c.layout == "shuffled":
            v = rng.permutation(v)
        elif c.layout == "holes":
            holes = rng.random(c.N) < 1 / 6
            v = np.where(holes, rng.choice([-1, -1, c.B, c.B + 7, -2 ** 31, 2 ** 31 - 1], c.N), v)
    return v.astype(np.int32)


def rows_of(c, seed=0):
    """(x float32 [N,3], origin float32 [B,3]) of a case as numpy: x = origin[view] + a direction uniform on the sphere times a
    length in [0.5, 3] (rows without a view sit around the first origin)."""
    rng = np.random.default_rng(2000 * seed + 7 * c.N + 13 * c.degree + c.B + 1)
    origin = rng.uniform(-2.0, 2.0, (c.B, 3))
    d = rng.standard_normal((c.N, 3))
    d /= np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-3)
    w = d * rng.uniform(0.5, 3.0, (c.N, 1))
    v = views_of(c, seed).astype(np.int64)
    base = origin[np.where((v >= 0) & (v < c.B), v, 0)] if c.form == "views" else (origin[0] if c.form == "single" else 0.0)
    return (w + base).astype(np.float32), origin.astype(np.float32)
