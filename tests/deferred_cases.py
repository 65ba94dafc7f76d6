"""The deferred-shading unit (csrc/dmr_interp.hip: interpolate_fused, composite_values_fused): which kernel instantiation a call
reaches, and the case tables of its GPU tests (tests/test_deferred_gpu.py).  No GPU code: the GPU tests import their tables
from here, and tests/test_deferred_cpu.py checks, without a GPU, that the tables together reach every instantiation the unit
compiles.  In shading_cases.py's role, and on its frames and sizes.
"""
from collections import namedtuple

from shading_cases import EDGE_FRAMES, FRAME, MERGE_FRAME, NEW_FRAME, SIZES, KMAXES, kmax_of, smallest_k, vec_of  # noqa: F401

# ---------------------------------------------------------------------------
# The host dispatch of dmr_interp.hip, restated.  DISPATCH_LINES holds the lines this mirrors; tests/test_deferred_cpu.py fails
# when one of them is no longer in the file exactly once: then this follows the new dispatch.  (with_kmax and shade_vec are
# dmr_shade_common.hpp's, restated in shading_cases.kmax_of / vec_of and pinned by tests/test_shading_coverage_cpu.py.)
# COMMON_DISPATCH_LINES: the same for what this unit and the packed one (tests/packed_cases.py) take from COMMON_HEADER.
# ---------------------------------------------------------------------------
DEFER_MAX_C = 256
COMMON_HEADER = "dmr_deferred_common.hpp"
COMMON_DISPATCH_LINES = [
    "p.vec = shade_vec(C, vert_attrs);",
]
DISPATCH_LINES = [
    "constexpr int DEFER_MAX_C = 256;",
    "if (C <= 4) k_interpolate_fragments<4><<<rows, block, 0, st>>>(p, out);",
    "else k_interpolate_fragments<8><<<rows, block, 0, st>>>(p, out);",
    "if (C <= 4) k_interpolate_fragments_backward<4><<<groups, block, 0, st>>>(p, grad_out, dL_dvert_attrs, dL_dbary);",
    "else k_interpolate_fragments_backward<8><<<groups, block, 0, st>>>(p, grad_out, dL_dvert_attrs, dL_dbary);",
    "if (C <= 4) k_composite_values<4><<<rows, block, 0, st>>>(p, image, T);",
    "else k_composite_values<16><<<rows, block, 0, st>>>(p, image, T);",
    "if (p.C <= 4) k_composite_values_backward<KMAX, 4><<<",
    "else k_composite_values_backward<KMAX, 8><<<",
    "with_kmax(K, [&](auto kmax) {",
    "launch_values_backward<decltype(kmax)::value>(p, st, grad_image, grad_T, dop, dval, dsc);",
]


def interp_ch(C):
    """dmr_interpolate_fragments, dmr_interpolate_packed and their backwards: if (C <= 4) <4> else <8>."""
    return 4 if C <= 4 else 8


def values_forward_ch(C):
    """dmr_composite_values and dmr_composite_values_packed: if (C <= 4) <4> else <16>."""
    return 4 if C <= 4 else 16


def values_backward_ch(C):
    """launch_values_backward and launch_packed_values_backward: if (p.C <= 4) <KMAX, 4> else <KMAX, 8>."""
    return 4 if C <= 4 else 8


# One forward + backward of BOTH pairs as the dispatch sees it.  aligned: the base of vert_attrs is 16-byte aligned.
Reach = namedtuple("Reach", "K C aligned")


def reach(K, C, aligned=True):
    assert 1 <= K <= 32 and 1 <= C <= DEFER_MAX_C
    return Reach(K, C, aligned)


def instantiations(cases):
    """The set of (kernel name, template arguments, vec) the calls `cases` (Reach) run; vec is None where no float4 rule applies."""
    out = set()
    for r in cases:
        v = vec_of(r.C, r.aligned)
        out.add(("k_interpolate_fragments", (interp_ch(r.C),), v))
        out.add(("k_interpolate_fragments_backward", (interp_ch(r.C),), v))
        out.add(("k_composite_values", (values_forward_ch(r.C),), None))
        out.add(("k_composite_values_backward", (kmax_of(r.K), values_backward_ch(r.C)), None))
    return out


def every_instantiation():
    """All of them.  vec = 1 needs C % 4 == 0: with C <= 4 that is C = 4."""
    full = {(k, (ch,), v) for k in ("k_interpolate_fragments", "k_interpolate_fragments_backward") for ch in (4, 8) for v in (0, 1)}
    full |= {("k_composite_values", (ch,), None) for ch in (4, 16)}
    full |= {("k_composite_values_backward", (k, ch), None) for k in KMAXES for ch in (4, 8)}
    return full


# ---------------------------------------------------------------------------
# The tables
# ---------------------------------------------------------------------------
LISTS_K = (1, 5, 32)       # test_caller_made_lists: K x C x size (x with_scale for the blend) on FRAME
LISTS_C = (1, 3, 5, 35)
MATRIX_K = (4, 8, 9, 16, 17, 32)   # test_instantiation_matrix on NEW_FRAME: every KMAX at K == KMAX, 16 and 32 at their smallest K too
MATRIX_C = (4, 8, 16, 20, 3)       # float4 at CH 4, one CH 8 walk, one CH 16 walk, a cut CH 16 walk, scalar
BOTH_SIZES = tuple(SIZES)
# (K, C, size): the sizes alternate over the matrix, so that every K and every C meets both; then DEFER_MAX_C and the scalar below it
MATRIX = [(K, C, BOTH_SIZES[(i + j) % 2]) for i, K in enumerate(MATRIX_K) for j, C in enumerate(MATRIX_C)]
MATRIX += [(4, 256, "table_overflow"), (5, 255, "shared_keys")]
IDENTITY = [(5, 3, "shared_keys"), (8, 8, "table_overflow")]   # test_identity_on_the_device: K, C, size on FRAME
ONLY_SOME = (5, 5, "shared_keys")                              # test_only_some_gradients_wanted
POISON = (5, 3, "shared_keys")                                 # test_empty_slot_values_are_not_read: K, C, size ...
POISON_FRAME = (1, 4, 15)    # ... inside ONE workgroup of either lane mapping (64 x 4 and 16 x 16 pixels): every face's sum is then
#                              one table cell and one atomic, so two runs are bit-equal
BAD_ROWS = (5, 5, "shared_keys")                               # test_face_with_a_vertex_out_of_range, test_non_finite_upstreams
EDGE_K, EDGE_C = 5, 3                                          # test_frames on EDGE_FRAMES
MERGE_C = 4                                                    # test_merge_levels on MERGE_FRAME (K, F, P: shading_cases.MERGE_*)
GRAPH = (5, 35, "table_overflow")                              # test_graph_capture


def tables():
    """Every table above as the calls it makes: {name: [Reach]}."""
    from shading_cases import MERGE_K
    t = {}
    t["caller_made_lists"] = [reach(K, C) for K in LISTS_K for C in LISTS_C]
    t["matrix"] = [reach(K, C) for K, C, _ in MATRIX]
    t["misaligned"] = [reach(K, C, False) for K, C, _ in MATRIX if C % 4 == 0]
    t["identity"] = [reach(K, C) for K, C, _ in IDENTITY]
    t["only_some"] = [reach(*ONLY_SOME[:2])]
    t["poison"] = [reach(*POISON[:2])]
    t["bad_rows"] = [reach(*BAD_ROWS[:2])]
    t["frames"] = [reach(EDGE_K, EDGE_C) for _ in EDGE_FRAMES]
    t["merge"] = [reach(MERGE_K, MERGE_C)]
    t["graph"] = [reach(*GRAPH[:2])]
    return t
