"""The packed deferred-shading unit (csrc/dmr_packed.hip: pack_slots_fused, interpolate_packed_fused,
composite_values_packed_fused): which kernel instantiation a call reaches, and the case tables of its GPU tests
(tests/test_packed_gpu.py).  No GPU code: the GPU tests import their tables from here, and tests/test_packed_cpu.py checks,
without a GPU, that the tables together reach every instantiation the unit compiles.  In deferred_cases.py's role, and on
shading_cases.py's frames and sizes.
"""
from collections import namedtuple

from deferred_cases import COMMON_DISPATCH_LINES, COMMON_HEADER, interp_ch, values_backward_ch, values_forward_ch  # noqa: F401
from shading_cases import EDGE_FRAMES, FRAME, NEW_FRAME, SIZES, KMAXES, kmax_of, smallest_k, vec_of  # noqa: F401

# ---------------------------------------------------------------------------
# The host dispatch of dmr_packed.hip, restated.  DISPATCH_LINES holds the lines this mirrors; tests/test_packed_cpu.py fails
# when one of them is no longer in the file exactly once: then this follows the new dispatch.  (with_kmax and shade_vec are
# dmr_shade_common.hpp's, restated in shading_cases.kmax_of / vec_of and pinned by tests/test_shading_coverage_cpu.py.)
# The channel chunks (interp_ch, values_forward_ch, values_backward_ch) are the dense unit's, and so are deferred_cases' functions:
# the lines below pin that this unit's dispatch has the same thresholds.  COMMON_DISPATCH_LINES: what both take from COMMON_HEADER.
# ---------------------------------------------------------------------------
PACKED_MAX_C = 256
PACK_SLOTS = 2048    # slots of the flattened lists per workgroup of k_pack_count / k_pack_write
PACK_SCAN = 256      # workgroups k_pack_scan's one workgroup scans at a time
DISPATCH_LINES = [
    "constexpr int PACKED_MAX_C = 256;",
    "constexpr int PACK_PASSES = 8, PACK_SLOTS = 256 * PACK_PASSES, PACK_SCAN = 256;",
    "const int groups = (int)((slots + PACK_SLOTS - 1) / PACK_SLOTS);",
    "p.rvec = shade_vec(C, values);",
    "if (C <= 4) k_interpolate_packed<4, false><<<rows, block, 0, st>>>(p, main_groups, out);",
    "constexpr int PLAIN_MAX_C = 8, STAGE_MAX_C = 32, STAGE_ROW = STAGE_MAX_C + 1;",
    "bool via_lds = C > PLAIN_MAX_C && C <= STAGE_MAX_C;",
    "else if (via_lds) k_interpolate_packed<8, true><<<rows, block, 0, st>>>(p, main_groups, out);",
    "else k_interpolate_packed<8, false><<<rows, block, 0, st>>>(p, main_groups, out);",
    "if (C <= 4) k_interpolate_packed_backward<4><<<groups, block, 0, st>>>(p, grad_out, dL_dvert_attrs, dL_dbary);",
    "else k_interpolate_packed_backward<8><<<groups, block, 0, st>>>(p, grad_out, dL_dvert_attrs, dL_dbary);",
    "if (C <= 4) k_composite_values_packed<4><<<rows, block, 0, st>>>(p, image, T);",
    "else k_composite_values_packed<16><<<rows, block, 0, st>>>(p, image, T);",
    "if (p.C <= 4) k_composite_values_packed_backward<KMAX, 4><<<",
    "else k_composite_values_packed_backward<KMAX, 8><<<",
    "with_kmax(K, [&](auto kmax) {",
    "launch_packed_values_backward<decltype(kmax)::value>(p, st, grad_image, grad_T, dop, dval, dsc);",
]


def pack_groups(slots):
    """dmr_pack_slots: groups = ceil(B K H W / PACK_SLOTS) workgroups count and write; one workgroup scans them PACK_SCAN at a time."""
    return (slots + PACK_SLOTS - 1) // PACK_SLOTS


PLAIN_MAX_C, STAGE_MAX_C = 8, 32


def interp_via_lds(C):
    """dmr_interpolate_packed's store shape: rows transposed through LDS where a row is more than one chunk and fits the stage."""
    return PLAIN_MAX_C < C <= STAGE_MAX_C


# One forward + backward of BOTH pairs as the dispatch sees it.  aligned: the base of vert_attrs (interpolate: p.vec) and of
# values (composite: p.rvec) is 16-byte aligned; the tensors the binding allocates always are.
Reach = namedtuple("Reach", "K C aligned")


def reach(K, C, aligned=True):
    assert 1 <= K <= 32 and 1 <= C <= PACKED_MAX_C
    return Reach(K, C, aligned)


def instantiations(cases):
    """The set of (kernel name, template arguments, float4 access) the calls `cases` (Reach) run."""
    out = set()
    for r in cases:
        v = vec_of(r.C, r.aligned)
        out.add(("k_interpolate_packed", (interp_ch(r.C), interp_via_lds(r.C)), v))
        out.add(("k_interpolate_packed_backward", (interp_ch(r.C),), v))
        out.add(("k_composite_values_packed", (values_forward_ch(r.C),), v))
        out.add(("k_composite_values_packed_backward", (kmax_of(r.K), values_backward_ch(r.C)), v))
    return out


def every_instantiation():
    """All of them, each with scalar and with float4 access.  float4 needs C % 4 == 0: with C <= 4 that is C = 4."""
    full = {("k_interpolate_packed", t, v) for t in ((4, False), (8, False), (8, True)) for v in (0, 1)}
    full |= {("k_interpolate_packed_backward", (ch,), v) for ch in (4, 8) for v in (0, 1)}
    full |= {("k_composite_values_packed", (ch,), v) for ch in (4, 16) for v in (0, 1)}
    full |= {("k_composite_values_packed_backward", (k, ch), v) for k in KMAXES for ch in (4, 8) for v in (0, 1)}
    return full


# ---------------------------------------------------------------------------
# The tables
# ---------------------------------------------------------------------------
# pack_slots_fused against pack_slots: (B, K, H, W) -- one slot; one less than, exactly and one more than a workgroup's share;
# at least three workgroups; more first-level workgroups than the scanning workgroup takes at a time (258 > PACK_SCAN)
PACK_SHAPES = [(1, 1, 1, 1), (1, 1, 23, 89), (1, 2, 32, 32), (1, 1, 3, 683), (2, 5, 24, 40), (1, 32, 128, 129)]
PACK_FILLS = ("mixed", "all_empty", "all_used")   # 15 % -1 and 10 % ids past F; every slot -1; every slot a face
PACK_F = 7

LISTS_K = (1, 5, 32)       # test_caller_made_lists: K x C x size on FRAME, face_scale alternating
LISTS_C = (1, 3, 4, 5, 35)
BOTH_SIZES = tuple(SIZES)
WIDE = [(1, 255, "shared_keys"), (5, 256, "table_overflow"), (32, 255, "table_overflow"), (32, 256, "shared_keys")]  # ... on NEW_FRAME
MATRIX_K = (4, 8, 9, 16, 17)   # test_instantiation_matrix on NEW_FRAME: every KMAX at K == KMAX (32: LISTS_K), 16 and 32 at their smallest K too
MATRIX_C = (4, 8, 3, 20)       # float4 at CH 4, float4 at CH 8 / 16, scalar, rows of three chunks staged through LDS
MATRIX = [(K, C, BOTH_SIZES[(i + j) % 2]) for i, K in enumerate(MATRIX_K) for j, C in enumerate(MATRIX_C)]
CAPACITY = (5, 5, "shared_keys")        # test_capacity: above and below the count; K, C, size on FRAME ...
CAPACITY_C = (5, 17)                    # ... at these C: the plain stores, and rows staged through LDS
HAND_MADE = [(5, 5, "shared_keys"), (5, 16, "table_overflow"), (5, 27, "shared_keys")]   # test_rows_in_another_order
OTHER_F = (5, 4, "shared_keys")         # test_packed_for_a_larger_f
BAD_ROWS = (5, 5, "shared_keys")        # test_face_with_a_vertex_out_of_range
DENSE = [(5, 3, "shared_keys"), (8, 8, "table_overflow"), (5, 16, "shared_keys"), (32, 35, "shared_keys")]   # test_against_the_dense_unit on FRAME
EDGE_K, EDGE_C = 5, 3                   # test_frames on NEW_FRAME and EDGE_FRAMES
GRAPH = (5, 35, "table_overflow")       # test_graph_replay


def tables():
    """Every table above as the calls it makes: {name: [Reach]}."""
    t = {}
    t["caller_made_lists"] = [reach(K, C) for K in LISTS_K for C in LISTS_C]
    t["wide"] = [reach(K, C) for K, C, _ in WIDE]
    t["matrix"] = [reach(K, C) for K, C, _ in MATRIX]
    t["misaligned"] = [reach(K, C, False) for K, C, _ in MATRIX if C % 4 == 0]
    t["capacity"] = [reach(CAPACITY[0], C) for C in CAPACITY_C]
    t["hand_made"] = [reach(K, C) for K, C, _ in HAND_MADE]
    t["other_f"] = [reach(*OTHER_F[:2])]
    t["bad_rows"] = [reach(*BAD_ROWS[:2])]
    t["dense"] = [reach(K, C) for K, C, _ in DENSE]
    t["frames"] = [reach(EDGE_K, EDGE_C) for _ in [NEW_FRAME] + EDGE_FRAMES]
    t["graph"] = [reach(*GRAPH[:2])]
    return t
