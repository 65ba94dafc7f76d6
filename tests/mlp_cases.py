"""The row MLP unit (csrc/dmr_mlp.hip: fragments.mlp_rows_fused): which kernel instantiation a call reaches, the launch
constants the shapes of its GPU tests are built from, and the case table of tests/test_mlp_gpu.py.  No GPU code: the GPU
tests import the table from here, and tests/test_mlp_cpu.py checks, without a GPU, that it reaches every instantiation the
unit compiles and that the dispatch lines restated here are still in the unit.  In packed_cases.py's role.
"""
from collections import namedtuple

# ---------------------------------------------------------------------------
# The host dispatch of dmr_mlp.hip, restated.  DISPATCH_LINES holds the lines this mirrors; tests/test_mlp_cpu.py fails when
# one of them is no longer in the file exactly once: then this follows the new dispatch.  What the row units take from the
# shared csrc/dmr_rows_common.* is restated once, in tests/row_units.py (COMMON_DISPATCH_LINES; this unit fills nothing).
# ---------------------------------------------------------------------------
HIDDEN = (16, 32, 64)
MAX_CIN, MAX_COUT = 64, 16
FWD_THREADS, FWD_MAX_GROUPS, BWD_MAX_GROUPS = 256, 1024, 512
DISPATCH_LINES = [
    "constexpr int MLP_MAX_CIN = 64, MLP_OUT = 16;",
    "constexpr int MLP_FWD_THREADS = 256, MLP_FWD_MAX_GROUPS = 1024, MLP_BWD_MAX_GROUPS = DMR_MLP_MAX_GROUPS;",
    "constexpr int mlp_bwd_threads(int hd, int nh) { return hd == 64 && nh == 2 ? 128 : 256; }",
    "with_one_of<16, 32, 64>(Hd, [&](auto hd) {",
    "with_one_of<1, 2>(n_hidden, [&](auto nh) {",
    "if (vec) f(hd, nh, std::true_type());",
    "else f(hd, nh, std::false_type());",
    "mlp_with_shape(Hd, n_hidden, shade_vec(Cin, x) != 0, [&](auto hd, auto nh, auto vec) {",
    "const bool vec = shade_vec(Cin, x) && (!dL_dx || shade_vec(Cin, dL_dx));",
    "mlp_with_shape(Hd, n_hidden, vec, [&](auto hd, auto nh, auto v) {",
    "const RowsGrid g = rows_grid(N, MLP_FWD_THREADS, MLP_FWD_MAX_GROUPS);",
    "const dim3 groups((unsigned)g.groups), block(MLP_FWD_THREADS);",
    "const RowsGrid g = rows_grid(N, mlp_bwd_threads(Hd, n_hidden), MLP_BWD_MAX_GROUPS);",
    "const int go = rows_backward_prologue(name, N, grad_out, own, dL_dx, want_w);",
]
HEADER_LINES = ["#define DMR_MLP_MAX_GROUPS 512"]   # ... of include/dmesh_renderer_amd_mlp.h


def bwd_threads(hd, nh):
    """The rows of a backward workgroup's tile (mlp_bwd_threads)."""
    return 128 if hd == 64 and nh == 2 else 256


def vec_of(cin, aligned):
    """shade_vec(Cin, x): rows of x (and of dL_dx, which the binding allocates aligned) are read as float4."""
    return bool(cin % 4 == 0 and aligned)


# One forward + backward as the dispatch sees it.  aligned: x's base is 16-byte aligned.
Case = namedtuple("Case", "N Cin Hd nh Cout act oact bias aligned")


def case(N, Cin, Hd, nh, Cout, act="relu", oact="none", bias=True, aligned=True):
    assert N >= 0 and 1 <= Cin <= MAX_CIN and Hd in HIDDEN and nh in (1, 2) and 1 <= Cout <= MAX_COUT
    return Case(N, Cin, Hd, nh, Cout, act, oact, bias, aligned)


def instantiations(cases):
    """The set of (kernel, (Hd, hidden layers), float4 row loads) the calls `cases` run (N = 0 launches only the reduction)."""
    out = set()
    for c in cases:
        v = vec_of(c.Cin, c.aligned)
        if c.N > 0:
            out.add(("k_mlp_rows", (c.Hd, c.nh), v))
            out.add(("k_mlp_rows_backward", (c.Hd, c.nh), v))
        out.add(("k_mlp_reduce", (c.Hd, c.nh), None))
    return out


def every_instantiation():
    full = {(k, (hd, nh), v) for k in ("k_mlp_rows", "k_mlp_rows_backward") for hd in HIDDEN for nh in (1, 2) for v in (False, True)}
    return full | {("k_mlp_reduce", (hd, nh), None) for hd in HIDDEN for nh in (1, 2)}


# ---------------------------------------------------------------------------
# The table: the smallest shapes at which a kernel can go wrong, not the full product.
# ---------------------------------------------------------------------------
def _table():
    t = []
    # every Hd x hidden layers, with scalar and with float4 row loads, N around a wave, both widths of the output loop
    for i, hd in enumerate(HIDDEN):
        for nh in (1, 2):
            t.append(case((63, 65, 257)[i], (3, 5, 33)[i], hd, nh, (3, 1, 16)[i], act=("relu", "tanh")[nh - 1], oact=("none", "sigmoid")[i % 2]))
            t.append(case((64, 1000, 257)[i], (4, 32, 64)[i], hd, nh, (4, 16, 3)[i], act=("tanh", "relu")[nh - 1], oact=("sigmoid", "none")[i % 2],
                          bias=bool((i + nh) % 2)))
    # N = 0 and 1; Cin = 1; one row more than a backward workgroup's tile (both tile sizes)
    t += [case(0, 3, 16, 1, 3), case(0, 4, 64, 2, 4, oact="sigmoid"), case(1, 1, 16, 2, 1, act="tanh"), case(1, 64, 64, 1, 16)]
    t += [case(bwd_threads(64, 2) + 1, 5, 64, 2, 3, act="tanh"), case(bwd_threads(64, 1) + 1, 4, 64, 1, 4), case(bwd_threads(32, 2) + 1, 32, 32, 2, 4, bias=False)]
    # one tile more than the capped grids hold: the backward's (a workgroup takes a second tile), then the forward's
    t += [case(BWD_MAX_GROUPS * bwd_threads(16, 1) + 1, 3, 16, 1, 3, act="tanh"), case(BWD_MAX_GROUPS * bwd_threads(64, 2) + 1, 4, 64, 2, 1),
          case(FWD_MAX_GROUPS * FWD_THREADS + 1, 1, 16, 1, 1)]
    return t


TABLE = _table()
MISALIGNED = [c._replace(aligned=False) for c in TABLE if c.Cin % 4 == 0 and 0 < c.N <= 1000]   # x one float off a 16-byte boundary
N_ROWS = case(300, 5, 32, 2, 3, act="tanh")          # test_n_rows: the counts 0, below N, N, above N, negative
N_ROWS_VEC = case(300, 8, 64, 1, 4, oact="sigmoid")  # ... and with float4 rows
DEAD_UNIT = case(200, 4, 16, 1, 3)                   # a hidden unit of all-zero weights and zero bias: relu'(0) = 0
ONLY = case(130, 5, 16, 2, 3, act="tanh")            # each single gradient alone
GRAPH = case(700, 8, 32, 2, 3, act="tanh", oact="sigmoid")
CHAIN = dict(hidden=32, n_hidden=2, activation="tanh")   # the RowMLP of the chains on rendered lists (C = 3 -> 3)


def tables():
    """Every table above as the calls it makes: {name: [Case]}."""
    return {"table": TABLE, "misaligned": MISALIGNED, "n_rows": [N_ROWS, N_ROWS_VEC], "dead_unit": [DEAD_UNIT], "only": [ONLY], "graph": [GRAPH],
            "chain": [case(1, 3, CHAIN["hidden"], CHAIN["n_hidden"], 3, act=CHAIN["activation"])]}
