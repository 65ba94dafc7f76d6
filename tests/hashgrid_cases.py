"""The hash-grid unit (csrc/dmr_hashgrid.hip: fragments.hashgrid_rows_fused): which kernel instantiation a call reaches, the
launch constants the shapes of its GPU tests are built from, and the case tables of tests/test_hashgrid_gpu.py.  No GPU code:
the GPU tests import the tables from here, and tests/test_hashgrid_cpu.py checks, without a GPU, that they reach every
instantiation the unit compiles and that the dispatch lines restated here are still in the unit.  In mlp_cases.py's role.
"""
from collections import namedtuple

import numpy as np

from row_units import FILL_KERNEL

# ---------------------------------------------------------------------------
# The host dispatch of dmr_hashgrid.hip, restated.  DISPATCH_LINES holds the lines this mirrors; tests/test_hashgrid_cpu.py
# fails when one of them is no longer in the file exactly once: then this follows the new dispatch.  What the row units take
# from the shared csrc/dmr_rows_common.* is restated once, in tests/row_units.py (COMMON_DISPATCH_LINES, FILL_KERNEL).
# ---------------------------------------------------------------------------
FEATURES = (1, 2, 4, 8)
THREADS, MAX_GROUPS = 256, 1024
DISPATCH_LINES = [
    "constexpr int HG_MAX_L = DMR_HASHGRID_MAX_LEVELS, HG_THREADS = 256, HG_MAX_GROUPS = DMR_HASHGRID_MAX_GROUPS;",
    "with_one_of<1, 2, 4, 8>(F, [&](auto f) {  // (the 4 instantiations of the forward)",
    "with_one_of<1, 2, 4, 8>(F, [&](auto f) {  // (... the 12 of the backward)",
    "k_hashgrid_rows<FF, true><<<groups, block, 0, st>>>(p, g.tiles, y);",
    "with_wanted(dL_dx != nullptr, dL_dtable != nullptr, [&](auto wx, auto wt) {  // (an output that is not wanted is null)",
    "k_hashgrid_rows_backward<decltype(f)::value, decltype(wx)::value, decltype(wt)::value><<<groups, block, 0, st>>>(p, g.tiles, grad_out, dL_dx, dL_dtable);",
    "const dim3 groups((unsigned)g.groups), block(HG_THREADS);",
    "const int go = rows_backward_prologue(name, N, grad_out, nullptr, dL_dx, dL_dtable != nullptr);",
    "rows_fill_on(st, dL_dtable, (int64_t)p.off[HG_MAX_L] * F, 0u);",
]
TWICE = ("const RowsGrid g = rows_grid(N, HG_THREADS, HG_MAX_GROUPS);", "dim3 groups((unsigned)g.groups), block(HG_THREADS);")   # (both calls)
HEADER_LINES = ["#define DMR_HASHGRID_MAX_GROUPS 1024", "#define DMR_HASHGRID_MAX_LEVELS 16", "#define DMR_HASHGRID_MAX_CHANNELS 64"]

# One forward + backward as the dispatch sees it.  (R0, s): the grid's base resolution and per-level scale; order: how the rows
# follow each other ("ramp": along a line through the cube -- the wave merge and the LDS table; "random": uniform -- no merge,
# table refusals, direct atomics; "same": all N rows one point -- eight table rows per level take everything);
# want: which gradients the call asks for ("xt", "x", "t").
Case = namedtuple("Case", "N L F log2_T R0 s order want")


def case(N, L, F, log2_T, R0, s, order="ramp", want="xt"):
    assert N >= 0 and 1 <= L <= 16 and F in FEATURES and L * F <= 64 and order in ("ramp", "random", "same") and want in ("xt", "x", "t")
    return Case(N, L, F, log2_T, R0, float(s), order, want)


def instantiations(cases):
    """The set of (kernel, template arguments) the calls `cases` run (N = 0 launches only the zeroing kernel)."""
    out = set()
    for c in cases:
        if c.N > 0:
            out.add(("k_hashgrid_rows", (c.F, True)))
            out.add(("k_hashgrid_rows_backward", (c.F, "x" in c.want, "t" in c.want)))
        if "t" in c.want:
            out.add((FILL_KERNEL, ()))
    return out


def every_instantiation():
    full = {("k_hashgrid_rows", (f, True)) for f in FEATURES}
    full |= {("k_hashgrid_rows_backward", (f, wx, wt)) for f in FEATURES for wx, wt in ((True, True), (True, False), (False, True))}
    return full | {(FILL_KERNEL, ())}


# The three grids of the issue: (R0, s, L), with the share of uniform rows the boundary band leaves out below 3 %.
GRIDS = ((16, 2.0, 8), (4, 1.3819, 16), (2, 2.0, 12))


def _table():
    t = []
    # N around a wave and a workgroup's tile, L x F with L * F in {1, 8, 32, 64}; all levels dense (log2_T = 24 over small R)
    t += [case(0, 1, 1, 10, 4, 2), case(1, 1, 1, 10, 4, 2), case(63, 8, 1, 10, 2, 1.5), case(64, 2, 4, 12, 3, 3, "random"), case(65, 1, 8, 8, 5, 1)]
    t += [case(257, 16, 2, 10, 2, 1.35, "random"), case(257, 8, 4, 12, 4, 1.6), case(130, 16, 4, 11, 2, 1.4), case(257, 8, 8, 12, 3, 1.7, "random")]
    t += [case(300, 4, 2, 24, 2, 2), case(300, 4, 2, 24, 2, 2, "random")]
    # log2_T = 4: every level hashed, every corner colliding
    t += [case(257, 4, 2, 4, 2, 2), case(200, 2, 8, 4, 3, 5, "same")]
    # log2_T = 10 and 14 with the three grids: dense and hashed levels mixed, R up to 4096 (the hash's 32-bit wrap on the device)
    for log2_T in (10, 14):
        for i, (R0, s, L) in enumerate(GRIDS):
            t.append(case((1000, 700, 1000)[i], L, (2, 4, 1)[i], log2_T, R0, s, ("ramp", "random", "ramp")[i] if log2_T == 10 else ("random", "ramp", "same")[i]))
    # all rows identical: maximal contention on eight rows per level
    t += [case(1000, 8, 2, 12, 16, 2, "same")]
    # one workgroup tile more than the capped grid holds: a workgroup takes a second tile
    t += [case(MAX_GROUPS * THREADS + 1, 2, 1, 10, 8, 4), case(MAX_GROUPS * THREADS + 257, 1, 2, 8, 32, 1, "random")]
    return t


TABLE = _table()
ONLY = [case(130 + 70 * i, 3, f, 8, 3, 2.5, ("ramp", "random")[i % 2]) for i, f in enumerate(FEATURES)]   # each single gradient alone
MISALIGNED = [case(257, 8, 4, 12, 4, 1.6), case(100, 16, 2, 10, 2, 1.35, "random"), case(65, 3, 1, 8, 3, 2)]   # y one float off a 16-byte boundary
SPECIAL = case(0, 4, 2, 10, 4, 2)        # R = 4, 8 dense, 16, 32 hashed: powers of two, so a coordinate on a grid vertex is exact
N_ROWS = case(300, 8, 2, 10, 4, 1.5)     # the counts 0, below N, N, above N, negative
GRAPH = case(700, 8, 2, 12, 4, 1.6)
CHAIN = dict(n_levels=8, features=4, log2_table_size=12, base_resolution=4, per_level_scale=1.5, hidden=32)   # HashGrid -> RowMLP(32, 32, 3)


def tables():
    """Every table above as the calls it makes: {name: [Case]}."""
    only = [c._replace(want=w) for c in ONLY for w in ("xt", "x", "t")]
    return {"table": TABLE, "only": only, "misaligned": MISALIGNED, "special": [SPECIAL._replace(N=1)], "n_rows": [N_ROWS], "graph": [GRAPH],
            "chain": [case(1, CHAIN["n_levels"], CHAIN["features"], CHAIN["log2_table_size"], CHAIN["base_resolution"], CHAIN["per_level_scale"])]}


def rows_of(c, seed=0):
    """x float32 [N,3] of a case as numpy, inside the open unit cube."""
    rng = np.random.default_rng(1000 * seed + 7 * c.N + 13 * c.L + c.F + c.log2_T)
    if c.order == "random":
        return rng.uniform(0.0, 1.0, (c.N, 3)).astype(np.float32)
    if c.order == "same":
        return np.repeat(rng.uniform(0.1, 0.9, (1, 3)), c.N, axis=0).astype(np.float32)
    a, b = np.array([0.031, 0.912, 0.127]), np.array([0.957, 0.083, 0.871])
    s = np.linspace(0.0, 1.0, max(c.N, 1))[:c.N, None]
    return (a + (b - a) * s).astype(np.float32)


def boundary_band(x, resolutions):
    """bool [N]: rows that have, at some level, a coordinate within 8 * 2^-24 * R_l of a cell boundary -- eight half-spacings of
    float32 at the level's largest p, where floor(p) may differ between float32 and float64 and dL/dx jumps.  x float32 numpy."""
    u = np.clip(np.nan_to_num(x.astype(np.float64), nan=0.0, posinf=1.0, neginf=0.0), 0.0, 1.0)
    near = np.zeros(len(x), dtype=bool)
    for R in resolutions:
        p = u * R
        near |= (np.abs(p - np.round(p)) <= 8 * 2.0 ** -24 * R).any(axis=1)
    return near
