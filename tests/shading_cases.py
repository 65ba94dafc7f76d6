"""The fused shading units (csrc/dmr_shade.hip, csrc/dmr_texture.hip): which kernel instantiation a call reaches, and the case
tables of their GPU tests (tests/test_composite_fused_gpu.py, tests/test_composite_texture_gpu.py).  No GPU code: the GPU
tests import their tables from here, and tests/test_shading_coverage_cpu.py checks, without a GPU, that the tables together
reach every instantiation the two units compile.
"""
from collections import namedtuple

import torch as th

# ---------------------------------------------------------------------------
# The host dispatch, restated.  tests/test_shading_coverage_cpu.py holds the lines of the two .hip files and of their common
# header (csrc/dmr_shade_common.hpp) this mirrors (DISPATCH_LINES there) and fails when one of them is no longer in its file:
# then this follows the new dispatch.
# ---------------------------------------------------------------------------
FRAG_MAX_K = 32     # dmr_kernels.hpp
SHADE_MAX_C = 256   # dmr_shade.hip
TEX_MAX_C = 32      # dmr_texture.hip
KMAXES = (4, 8, 16, 32)


def kmax_of(K):
    """with_kmax of dmr_shade_common.hpp, which both backward calls launch through: if (K <= 4) <4> else if (K <= 8) <8> else
    if (K <= 16) <16> else <32>."""
    assert 1 <= K <= FRAG_MAX_K
    return 4 if K <= 4 else (8 if K <= 8 else (16 if K <= 16 else 32))


def smallest_k(kmax):
    """The smallest K that reaches KMAX = kmax."""
    return {4: 1, 8: 5, 16: 9, 32: 17}[kmax]


def shade_forward_ch(C):
    """dmr_composite_fragments: if (C <= 4) k_composite_fragments<4> else k_composite_fragments<16>."""
    return 4 if C <= 4 else 16


def shade_backward_ch(C):
    """launch_backward of dmr_shade.hip: if (p.C <= 4) <KMAX, 4> else <KMAX, 8>."""
    return 4 if C <= 4 else 8


def texture_forward_nch(C):
    """dmr_composite_texture: if (C <= 4) k_composite_texture<1> else k_composite_texture<TEX_CHUNKS> (TEX_MAX_C / 4 = 8)."""
    return 1 if C <= 4 else TEX_MAX_C // 4


def vec_of(C, aligned):
    """shade_vec of dmr_shade_common.hpp, as shade_params / tex_params call it: p.vec = C % 4 == 0 and a 16-byte aligned base
    of vert_attrs / texture."""
    return int(C % 4 == 0 and aligned)


def tex_of(texture_grad_wanted, image_upstream=True):
    """launch_backward of dmr_texture.hip: TEX = dtex && gi."""
    return bool(texture_grad_wanted and image_upstream)


# One forward + backward call as the dispatch sees it.  aligned: the base of vert_attrs / texture is 16-byte aligned; tex:
# the texture's gradient is wanted (texture unit; None for shade).  Every call of the tests has an image upstream.
Reach = namedtuple("Reach", "unit K C aligned tex")


def shade(K, C, aligned=True):
    assert 1 <= C <= SHADE_MAX_C
    return Reach("shade", K, C, aligned, None)


def texture(K, C, aligned=True, tex=True):
    assert 1 <= C <= TEX_MAX_C
    return Reach("texture", K, C, aligned, tex)


def instantiations(cases):
    """The set of (kernel name, template arguments, vec) the calls `cases` (Reach) run."""
    out = set()
    for r in cases:
        v = vec_of(r.C, r.aligned)
        if r.unit == "shade":
            out.add(("k_composite_fragments", (shade_forward_ch(r.C),), v))
            out.add(("k_composite_fragments_backward", (kmax_of(r.K), shade_backward_ch(r.C)), v))
        else:
            out.add(("k_composite_texture", (texture_forward_nch(r.C),), v))
            out.add(("k_composite_texture_backward", (kmax_of(r.K), tex_of(r.tex)), v))
    return out


def every_instantiation():
    """All of them.  vec = 1 needs C % 4 == 0: with C <= 4 (shade CH 4, texture NCH 1) that is C = 4."""
    full = {("k_composite_fragments", (ch,), v) for ch in (4, 16) for v in (0, 1)}
    full |= {("k_composite_fragments_backward", (k, ch), v) for k in KMAXES for ch in (4, 8) for v in (0, 1)}
    full |= {("k_composite_texture", (nch,), v) for nch in (1, 8) for v in (0, 1)}
    full |= {("k_composite_texture_backward", (k, tex), v) for k in KMAXES for tex in (True, False) for v in (0, 1)}
    return full


def one_float_in(t):
    """`t`'s values in a contiguous view that starts one float into a larger buffer of t's device: the binding's
    .contiguous() keeps its pointer, which is 4 bytes past a 16-byte boundary (the caller asserts data_ptr() % 16 == 4), so
    vec = 0 whatever C is."""
    buf = th.empty(t.numel() + 8, dtype=t.dtype, device=t.device)
    view = buf[1:1 + t.numel()].view(t.shape)
    view.copy_(t)
    return view


# ---------------------------------------------------------------------------
# Tables both units share
# ---------------------------------------------------------------------------
# (F, P or Pu).  shared_keys: many lanes of a wave share a key (the merge path, a handful of table cells).  table_overflow:
# a tile holds more distinct vertex / UV rows than the table's 560 slots; in the texture unit, with the 32 x 48 texture, it
# fills the texel table to its probe limit at K = 5 (about 1400 of the 1536 texels against 1408 cells) and past its size at
# K = 32 (1024 cells): rows leave with direct atomics
SIZES = {"shared_keys": (7, 9), "table_overflow": (6000, 9000)}
FRAME = (2, 24, 40)        # B, H, W of the first tables: partial tiles in both axes
NEW_FRAME = (1, 17, 33)    # of the instantiation matrix: six tiles, partial in both axes, 561 pixels (a cheap float64 model)
MERGE_FRAME = (1, 32, 32)  # of the merge-level lists
MERGE_K, MERGE_F, MERGE_P = 6, 5, 9
# whole tiles only / one live lane per workgroup (255 lanes with key -1 through every merge and barrier); at K = 5, C = 3
EDGE_FRAMES = [(1, 16, 32), (3, 1, 1)]
EDGE_FRAME_K, EDGE_FRAME_C = 5, 3

# ---------------------------------------------------------------------------
# Shade (composite_fused)
# ---------------------------------------------------------------------------
SHADE_K = (1, 5, 32)       # test_caller_made_lists: K x C x with_scale x size on FRAME
SHADE_C = (1, 3, 5, 35)
SHADE_ONLY_SOME = (5, 5, "shared_keys")       # test_only_some_gradients_wanted: K, C, size
SHADE_GRAPH = (5, 35, "table_overflow")       # test_graph_capture

BOTH_SIZES, BOTH = tuple(SIZES), (False, True)
# K, C, sizes, with_scale values: the instantiation matrix on NEW_FRAME
SHADE_MATRIX_ROWS = [
    (4, 4, BOTH_SIZES, BOTH),                 # <4,4> full, vec, forward CH 4 vec
    (8, 8, BOTH_SIZES, BOTH),                 # <8,8> full, vec, one backward walk exactly
    (9, 20, BOTH_SIZES, BOTH),                # <16,8>, vec, the forward's CH 16 guard at c0 = 16
    (16, 16, BOTH_SIZES, BOTH),               # <16,8> full, the forward's one whole CH 16 walk
    (16, 3, BOTH_SIZES, BOTH),                # <16,4> full, scalar
    (17, 4, BOTH_SIZES, BOTH),                # <32,4> at its smallest K, vec
    (4, 256, ("table_overflow",), (True,)),   # SHADE_MAX_C, vec: 16 forward walks, 32 backward walks
    (5, 255, ("shared_keys",), BOTH),         # the same scalar, the last walk 15 / 7 channels wide
]
SHADE_MATRIX = [(K, C, s, size) for K, C, sizes, scales in SHADE_MATRIX_ROWS for s in scales for size in sizes]
# K, C: vert_attrs one float into a buffer (vec = 0 with C % 4 == 0), beside the aligned call on the same values (vec = 1)
SHADE_MISALIGNED = [(16, 4), (12, 8), (32, 8)]
SHADE_MERGE_C = 4

# ---------------------------------------------------------------------------
# Texture (composite_texture_fused)
# ---------------------------------------------------------------------------
# K, C, texture (Ht, Wt), wrap, face_scale, uv_faces, size: every value of every axis, and both table regimes with both wraps
TEXTURE_CASES = [
    (1, 1, (1, 1), "clamp", False, False, "shared_keys"),
    (5, 3, (7, 13), "repeat", True, True, "shared_keys"),
    (32, 9, (7, 13), "clamp", False, True, "shared_keys"),
    (32, 1, (1, 1), "repeat", True, True, "table_overflow"),
    (1, 4, (7, 13), "repeat", False, False, "table_overflow"),
    (5, 4, (32, 48), "clamp", True, True, "table_overflow"),
    (5, 9, (32, 48), "repeat", False, True, "table_overflow"),
    (32, 3, (32, 48), "repeat", True, False, "table_overflow"),
    (5, 3, (32, 48), "clamp", True, False, "shared_keys"),
]
TEXTURE_ONLY_SOME = (5, 3, (7, 13), "shared_keys", True, "repeat")   # test_only_some_gradients_wanted: K, C, tex, size, uvf, wrap
TEXTURE_GRAPH = (5, 9, (32, 48), "table_overflow", True)             # test_graph_capture

# the same columns: the instantiation matrix on NEW_FRAME
TEXTURE_MATRIX = [
    (4, 4, (7, 13), "repeat", True, True, "shared_keys"),            # <4,true> full, vec, NCH 1
    (8, 8, (32, 48), "clamp", False, True, "table_overflow"),        # <8,true> full, NCH 8 with float4 loads
    (9, 5, (7, 13), "clamp", True, False, "shared_keys"),            # <16,true> at its smallest K; C in 5..8, two scalar chunks
    (16, 32, (32, 48), "repeat", True, True, "table_overflow"),      # <16,true> full, TEX_MAX_C: 12 288 keys, 1024 cells, nch 8
    (16, 1, (1, 1), "clamp", False, False, "table_overflow"),        # <16,true> full, one texel
    (17, 16, (7, 13), "repeat", False, True, "shared_keys"),         # <32,true> at its smallest K, vec
    (32, 32, (7, 13), "clamp", True, False, "table_overflow"),       # <32,true> full, TEX_MAX_C, vec
]
# K, C, texture, wrap, size (face_scale and uv_faces given): every gradient but the texture's -> TEX = false at every KMAX,
# scalar and float4
TEXTURE_NO_TEX_GRAD = [
    (4, 4, (7, 13), "repeat", "shared_keys"),
    (4, 6, (32, 48), "clamp", "table_overflow"),
    (8, 8, (7, 13), "clamp", "shared_keys"),
    (16, 16, (32, 48), "repeat", "table_overflow"),
    (16, 3, (7, 13), "clamp", "shared_keys"),
    (32, 32, (32, 48), "clamp", "table_overflow"),
    (32, 9, (7, 13), "repeat", "shared_keys"),
]
# K, C, texture, wrap: the texture one float into a buffer, beside the aligned call on the same values
TEXTURE_MISALIGNED = [(5, 4, (7, 13), "repeat"), (12, 8, (32, 48), "clamp"), (32, 32, (7, 13), "repeat")]
TEXTURE_MERGE = (8, (7, 13), "repeat")  # C, texture, wrap
TEXTURE_EDGE_FRAME = ((7, 13), "repeat")


def tables():
    """Every table above as the calls it makes: {name: [Reach]}.  *.new are this file's later additions."""
    t = {}
    t["shade.caller_made_lists"] = [shade(K, C) for K in SHADE_K for C in SHADE_C]
    t["shade.only_some"] = [shade(*SHADE_ONLY_SOME[:2])]
    t["shade.graph"] = [shade(*SHADE_GRAPH[:2])]
    t["shade.matrix"] = [shade(K, C) for K, C, _, _ in SHADE_MATRIX]
    t["shade.misaligned"] = [shade(K, C, a) for K, C in SHADE_MISALIGNED for a in (False, True)]
    t["shade.merge"] = [shade(MERGE_K, SHADE_MERGE_C)]
    t["shade.frames"] = [shade(EDGE_FRAME_K, EDGE_FRAME_C) for _ in EDGE_FRAMES]
    t["texture.caller_made_lists"] = [texture(c[0], c[1]) for c in TEXTURE_CASES]
    t["texture.only_some"] = [texture(*TEXTURE_ONLY_SOME[:2], tex=x) for x in (True, False)]  # all five / one of the other four alone
    t["texture.graph"] = [texture(*TEXTURE_GRAPH[:2])]
    t["texture.matrix"] = [texture(c[0], c[1]) for c in TEXTURE_MATRIX]
    t["texture.no_tex_grad"] = [texture(c[0], c[1], tex=False) for c in TEXTURE_NO_TEX_GRAD]
    t["texture.misaligned"] = [texture(c[0], c[1], a) for c in TEXTURE_MISALIGNED for a in (False, True)]
    t["texture.merge"] = [texture(MERGE_K, TEXTURE_MERGE[0])]
    t["texture.frames"] = [texture(EDGE_FRAME_K, EDGE_FRAME_C) for _ in EDGE_FRAMES]
    return t


# What the tables must reach beyond an instantiation: name -> predicate over a Reach (the edge inside an instantiation that a
# guard, an LDS offset or a table size decides).
EDGES = {
    "shade: float4 rows at C = 4 (one CH 4 walk)": lambda r: r.unit == "shade" and r.C == 4 and vec_of(r.C, r.aligned),
    "shade: one backward walk exactly, float4 (C = 8)": lambda r: r.unit == "shade" and r.C == 8 and vec_of(r.C, r.aligned),
    "shade: the forward's CH 16 guard cuts a float4 walk (C = 4 odd > 4)": lambda r: r.unit == "shade" and r.C > 4 and r.C % 8 == 4 and vec_of(r.C, r.aligned),
    "shade: one whole CH 16 walk, float4 (C = 16)": lambda r: r.unit == "shade" and r.C == 16 and vec_of(r.C, r.aligned),
    "shade: SHADE_MAX_C, float4": lambda r: r.unit == "shade" and r.C == SHADE_MAX_C and vec_of(r.C, r.aligned),
    "shade: SHADE_MAX_C - 1, scalar, a ragged last walk": lambda r: r.unit == "shade" and r.C == SHADE_MAX_C - 1,
    "shade: C % 4 == 0 on a misaligned base": lambda r: r.unit == "shade" and r.C % 4 == 0 and not r.aligned,
    "texture: NCH 8 with float4 loads": lambda r: r.unit == "texture" and r.C > 4 and vec_of(r.C, r.aligned),
    "texture: TEX_MAX_C against the 1024-cell texel table (KMAX 16)": lambda r: r.unit == "texture" and r.C == TEX_MAX_C and r.tex and kmax_of(r.K) == 16,
    "texture: TEX_MAX_C against the 1024-cell texel table (KMAX 32)": lambda r: r.unit == "texture" and r.C == TEX_MAX_C and r.tex and kmax_of(r.K) == 32,
    "texture: C in 5..8, two scalar chunks": lambda r: r.unit == "texture" and 5 <= r.C <= 7,
    "texture: one channel at KMAX 16": lambda r: r.unit == "texture" and r.C == 1 and kmax_of(r.K) == 16,
    "texture: C % 4 == 0 on a misaligned base, NCH 1": lambda r: r.unit == "texture" and r.C == 4 and not r.aligned,
    "texture: C % 4 == 0 on a misaligned base, NCH 8": lambda r: r.unit == "texture" and r.C > 4 and r.C % 4 == 0 and not r.aligned,
    "texture: TEX_MAX_C on a misaligned base": lambda r: r.unit == "texture" and r.C == TEX_MAX_C and not r.aligned,
}


# ---------------------------------------------------------------------------
# The binding's refusals (csrc/dmr_torch.cpp), below Python's checks: one wrong argument per call, at B, K, H, W = 1, 1, 1, 1,
# F = 1, P = Pu = 3, so that no call reaches a kernel.  The expected messages (tests/golden/shading_refusals.json, "binding")
# were copied from the source text of the binding before its list checks were merged, and compared on the GPU with a run of that
# binding over these cases: 82 calls, the same text in each.
# ---------------------------------------------------------------------------
def binding_refusals(unit, dev):
    """[(case, name of the call in _C, positional arguments)] for unit "shade" / "texture": every case through the forward
    call and through the backward call (need: nothing, so that a call that were not refused would return before its memsets).
    "visibility" / "deferred" / "packed": the tables of LIST_REFUSALS below."""
    if unit in LIST_REFUSALS:
        return LIST_REFUSALS[unit](dev)
    z = lambda *shape, dtype=th.float32: th.zeros(*shape, dtype=dtype, device=dev)
    good = dict(face=z(1, 1, 1, 1, dtype=th.int32), bary=z(1, 1, 2, 1, 1), corners=th.tensor([[0, 1, 2]], dtype=th.int32, device=dev),
                opacity=z(1) + 0.5, scale=None, grad_image=z(1, 3, 1, 1), grad_T=z(1, 1, 1, 1))
    if unit == "shade":
        good.update(attrs=z(3, 3))
        own, fwd, n_need = ("attrs",), "composite_fragments", 4
    else:
        good.update(uvs=z(3, 2), tex=z(2, 2, 3), wrap=0)
        own, fwd, n_need = ("uvs", "tex"), "composite_texture", 5
    cases = {
        "pix_to_face on the CPU": dict(face=good["face"].cpu()),
        "pix_to_face with three dimensions": dict(face=good["face"][0]),
        "bary of another shape": dict(bary=z(1, 1, 3, 1, 1)),
        "corner table [F,2]": dict(corners=good["corners"][:, :2]),
        "faces_opacity of another length": dict(opacity=z(2)),
        "K = 33": dict(face=z(1, 33, 1, 1, dtype=th.int32), bary=z(1, 33, 2, 1, 1)),
        "K = 0": dict(face=z(1, 0, 1, 1, dtype=th.int32), bary=z(1, 0, 2, 1, 1)),
        "empty fragment lists": dict(face=z(1, 1, 0, 1, dtype=th.int32), bary=z(1, 1, 2, 0, 1)),
        "face_scale of another shape": dict(scale=z(1, 2)),
        "bary on the CPU": dict(bary=good["bary"].cpu()),
        "face_scale on the CPU": dict(scale=th.zeros(1, 1)),
        "bary float64": dict(bary=good["bary"].double()),
        "pix_to_face int64": dict(face=good["face"].long()),
    }
    if unit == "shade":
        cases.update({"vert_attrs with one dimension": dict(attrs=z(3)), "C = 257": dict(attrs=z(3, 257)), "C = 0": dict(attrs=z(3, 0)),
                      "vert_attrs on the CPU": dict(attrs=th.zeros(3, 3))})
    else:
        cases.update({"vert_uvs [Pu,3]": dict(uvs=z(3, 3)), "texture with two dimensions": dict(tex=z(2, 2)), "C = 33": dict(tex=z(2, 2, 33)),
                      "no texel": dict(tex=z(0, 2, 3)), "wrap = 2": dict(wrap=2), "texture on the CPU": dict(tex=th.zeros(2, 2, 3)),
                      "bad C and bad wrap": dict(tex=z(2, 2, 33), wrap=2)})
    backward_only = {
        "need face_scale without face_scale": dict(need=(False,) * (n_need - 2) + (True, False)),
        "grad_image of another shape": dict(grad_image=z(1, 4, 1, 1)),
        "grad_T of another size": dict(grad_T=z(1, 1, 1, 2)),
        "grad_image on the CPU": dict(grad_image=th.zeros(1, 3, 1, 1)),
    }
    out = []
    for table, calls in ((cases, (fwd, fwd + "_backward")), (backward_only, (fwd + "_backward",))):
        for case, changes in table.items():
            a = dict(good, need=(False,) * n_need)
            a.update(changes)
            lists = [a["face"], a["bary"], a["corners"], a["opacity"]] + [a[k] for k in own] + [a["scale"]]
            for call in calls:
                tail = ([a["wrap"]] if unit == "texture" else []) + ([a["grad_image"], a["grad_T"], a["need"]] if call.endswith("_backward") else [])
                out.append((case, call, lists + tail))
    return out


# ---------------------------------------------------------------------------
# The same for the units over the lists alone (face_visibility*), the deferred pair (interpolate_fragments*, composite_values*)
# and its packed twin (pack_slots, interpolate_packed*, composite_values_packed*): F = 1, P = 3, C = 3, N = 1.  The expected
# messages (tests/golden/shading_refusals.json, "binding") are a record of the binding on the GPU before the six argument
# builders of these units were put together from shared checks.  A case's name starts with the family of calls it goes
# through; "A with B" is two wrong arguments, and says which check comes first.
# ---------------------------------------------------------------------------
def _refusals(good, families):
    """families: [(prefix, {call: argument names}, cases, backward_only)] -> [(case, call, positional arguments)]; a call whose
    name ends in _backward is a backward call, and takes the cases of both tables."""
    out = []
    for prefix, calls, cases, backward_only in families:
        for table, only_backward in ((cases, False), (backward_only, True)):
            for case, changes in table.items():
                a = dict(good)
                a.update(changes)
                for call, names in calls.items():
                    if call.endswith("_backward") or not only_backward:
                        out.append((prefix + ": " + case, call, [a[n] for n in names]))
    return out


def _visibility_refusals(dev):
    z = lambda *shape, dtype=th.float32: th.zeros(*shape, dtype=dtype, device=dev)
    good = dict(face=z(1, 1, 1, 1, dtype=th.int32), opacity=z(1) + 0.5, weight=None, coverage=False, grad_vis=z(1, 1), need=(False, False))
    calls = {"face_visibility": ("face", "opacity", "weight", "coverage"),
             "face_visibility_backward": ("face", "opacity", "weight", "grad_vis", "need")}
    k33 = dict(face=z(1, 33, 1, 1, dtype=th.int32))
    cases = {
        "pix_to_face on the CPU": dict(face=good["face"].cpu()),
        "pix_to_face with three dimensions": dict(face=good["face"][0]),
        "K = 33": k33,
        "K = 0": dict(face=z(1, 0, 1, 1, dtype=th.int32)),
        "empty fragment lists": dict(face=z(1, 1, 0, 1, dtype=th.int32)),
        "faces_opacity with two dimensions": dict(opacity=z(1, 1)),
        "pixel_weight of another shape": dict(weight=z(1, 1, 2)),
        "faces_opacity on the CPU": dict(opacity=th.zeros(1)),
        "pixel_weight on the CPU": dict(weight=th.zeros(1, 1, 1)),
        "pix_to_face int64": dict(face=good["face"].long()),
        "faces_opacity float64": dict(opacity=good["opacity"].double()),
        "K = 33 with faces_opacity with two dimensions": dict(k33, opacity=z(1, 1)),
        "empty fragment lists with faces_opacity with two dimensions": dict(face=z(1, 1, 0, 1, dtype=th.int32), opacity=z(1, 1)),
        "pixel_weight of another shape with faces_opacity on the CPU": dict(weight=z(1, 1, 2), opacity=th.zeros(1)),
    }
    backward_only = {
        "need pixel_weight without pixel_weight": dict(need=(False, True)),
        "grad_vis of another shape": dict(grad_vis=z(1, 2)),
        "grad_vis on the CPU": dict(grad_vis=th.zeros(1, 1)),
    }
    return _refusals(good, [("face_visibility", calls, cases, backward_only)])


def _interp_cases(z, good, k):
    """The cases both interpolate pairs share.  k(K): the lists of K slots as changes."""
    return {
        "pix_to_face on the CPU": dict(face=good["face"].cpu()),
        "pix_to_face with three dimensions": dict(face=good["face"][0]),
        "bary of another shape": dict(bary=z(1, 1, 3, 1, 1)),
        "faces [F,2]": dict(faces=good["faces"][:, :2]),
        "vert_attrs with one dimension": dict(attrs=z(3)),
        "K = 33": k(33),
        "K = 0": k(0),
        "C = 257": dict(attrs=z(3, 257)),
        "C = 0": dict(attrs=z(3, 0)),
        "bary on the CPU": dict(bary=good["bary"].cpu()),
        "faces on the CPU": dict(faces=good["faces"].cpu()),
        "vert_attrs on the CPU": dict(attrs=th.zeros(3, 3)),
        "bary float64": dict(bary=good["bary"].double()),
        "pix_to_face int64": dict(face=good["face"].long()),
        "K = 33 with C = 257": dict(k(33), attrs=z(3, 257)),
        "C = 257 with vert_attrs on the CPU": dict(attrs=th.zeros(3, 257)),
        "K = 0 with bary on the CPU": {n: (t.cpu() if n == "bary" else t) for n, t in k(0).items()},
    }


def _values_cases(z, good, k, values_of):
    """The cases both composite_values pairs share.  values_of(C): values of C channels."""
    return {
        "pix_to_face on the CPU": dict(face=good["face"].cpu()),
        "pix_to_face with three dimensions": dict(face=good["face"][0]),
        "faces_opacity with two dimensions": dict(opacity=z(1, 1)),
        "K = 33": k(33),
        "K = 0": k(0),
        "C = 257": dict(values=values_of(257)),
        "C = 0": dict(values=values_of(0)),
        "face_scale of another shape": dict(scale=z(1, 2)),
        "faces_opacity on the CPU": dict(opacity=th.zeros(1)),
        "values on the CPU": dict(values=good["values"].cpu()),
        "face_scale on the CPU": dict(scale=th.zeros(1, 1)),
        "values float64": dict(values=good["values"].double()),
        "K = 33 with C = 257": dict(k(33), values=values_of(257) if good["values"].dim() == 2 else z(1, 33, 257, 1, 1)),
        "C = 257 with faces_opacity on the CPU": dict(values=values_of(257), opacity=th.zeros(1)),
    }


def _values_backward_only(z):
    """The cases of both composite_values backward calls alone."""
    return {
        "need face_scale without face_scale": dict(need3=(False, False, True)),
        "grad_image of another shape": dict(grad_image=z(1, 4, 1, 1)),
        "grad_T of another size": dict(grad_T=z(1, 1, 1, 2)),
        "grad_image on the CPU": dict(grad_image=th.zeros(1, 3, 1, 1)),
    }


def _deferred_refusals(dev):
    z = lambda *shape, dtype=th.float32: th.zeros(*shape, dtype=dtype, device=dev)
    iz = lambda *shape: z(*shape, dtype=th.int32)
    good = dict(face=iz(1, 1, 1, 1), bary=z(1, 1, 2, 1, 1), faces=th.tensor([[0, 1, 2]], dtype=th.int32, device=dev), attrs=z(3, 3),
                opacity=z(1) + 0.5, values=z(1, 1, 3, 1, 1), scale=None, grad_out=z(1, 1, 3, 1, 1), grad_image=z(1, 3, 1, 1),
                grad_T=z(1, 1, 1, 1), need2=(False, False), need3=(False, False, False))
    interp_calls = {"interpolate_fragments": ("face", "bary", "faces", "attrs"),
                    "interpolate_fragments_backward": ("face", "bary", "faces", "attrs", "grad_out", "need2")}
    values_calls = {"composite_values": ("face", "opacity", "values", "scale"),
                    "composite_values_backward": ("face", "opacity", "values", "scale", "grad_image", "grad_T", "need3")}
    interp = _interp_cases(z, good, lambda K: dict(face=iz(1, K, 1, 1), bary=z(1, K, 2, 1, 1)))
    interp["empty fragment lists"] = dict(face=iz(1, 1, 0, 1), bary=z(1, 1, 2, 0, 1))
    interp_backward = {"grad_out of another shape": dict(grad_out=z(1, 1, 4, 1, 1)), "grad_out on the CPU": dict(grad_out=th.zeros(1, 1, 3, 1, 1))}
    values = _values_cases(z, good, lambda K: dict(face=iz(1, K, 1, 1), values=z(1, K, 3, 1, 1)), lambda C: z(1, 1, C, 1, 1))
    values.update({
        "values of another shape": dict(values=z(1, 1, 3, 1, 2)),
        "values with four dimensions": dict(values=z(1, 3, 1, 1)),
        "empty fragment lists": dict(face=iz(1, 1, 0, 1), values=z(1, 1, 3, 0, 1)),
        "empty fragment lists with face_scale of another shape": dict(face=iz(1, 1, 0, 1), values=z(1, 1, 3, 0, 1), scale=z(1, 2)),
    })
    return _refusals(good, [("interpolate_fragments", interp_calls, interp, interp_backward),
                            ("composite_values", values_calls, values, _values_backward_only(z))])


def _packed_refusals(dev):
    z = lambda *shape, dtype=th.float32: th.zeros(*shape, dtype=dtype, device=dev)
    iz = lambda *shape: z(*shape, dtype=th.int32)
    good = dict(face=iz(1, 1, 1, 1), bary=z(1, 1, 2, 1, 1), row=iz(1, 1, 1, 1), n_used=iz(1) + 1, faces=th.tensor([[0, 1, 2]], dtype=th.int32, device=dev),
                attrs=z(3, 3), opacity=z(1) + 0.5, values=z(1, 3), scale=None, F=1, capacity=1, N=1, grad_out=z(1, 3), grad_image=z(1, 3, 1, 1),
                grad_T=z(1, 1, 1, 1), need2=(False, False), need3=(False, False, False))
    # 2^31 slots in one element of memory: the size checks come before anything makes a tensor contiguous
    huge = lambda t: t.expand(2 ** 16, 1, 2 ** 15, 1)
    lists = {
        "pix_to_face on the CPU": dict(face=good["face"].cpu()),
        "pix_to_face with three dimensions": dict(face=good["face"][0]),
        "pix_to_face int64": dict(face=good["face"].long()),
    }
    with_row = {
        "row of another shape": dict(row=iz(1, 1, 1, 2)),
        "row with three dimensions": dict(row=iz(1, 1, 1)),
        "row on the CPU": dict(row=good["row"].cpu()),
        "row int64": dict(row=good["row"].long()),
        "row of another shape with K = 33": dict(face=iz(1, 33, 1, 1)),
    }
    n_used = {
        "n_used with two elements": dict(n_used=iz(2)),
        "n_used on the CPU": dict(n_used=good["n_used"].cpu()),
        "n_used with two elements with K = 33": dict(face=iz(1, 33, 1, 1), row=iz(1, 33, 1, 1), n_used=iz(2)),
    }
    pack = dict(lists)
    pack.update({
        "K = 33": dict(face=iz(1, 33, 1, 1)),
        "K = 0": dict(face=iz(1, 0, 1, 1)),
        "empty fragment lists": dict(face=iz(1, 1, 0, 1)),
        "B K H W = 2^31": dict(face=huge(good["face"])),
        "F = -1": dict(F=-1),
        "F = 2^31": dict(F=2 ** 31),
        "capacity = -1": dict(capacity=-1),
        "K = 33 with F = -1": dict(face=iz(1, 33, 1, 1), F=-1),
        "F = -1 with capacity = -1": dict(F=-1, capacity=-1),
    })
    k_interp = lambda K: dict(face=iz(1, K, 1, 1), bary=z(1, K, 2, 1, 1), row=iz(1, K, 1, 1))
    interp = _interp_cases(z, good, k_interp)
    interp.update(with_row)
    interp.update(n_used)
    interp.update({
        "empty fragment lists": dict(face=iz(1, 1, 0, 1), bary=z(1, 1, 2, 0, 1), row=iz(1, 1, 0, 1)),
        "B K H W = 2^31": dict(face=huge(good["face"]), row=huge(good["row"])),
        "rows = -1": dict(N=-1, grad_out=z(3)),  # (the backward call takes its rows from grad_out, and -1 when that is no [N,C])
        "bary of another shape with row on the CPU": dict(bary=z(1, 1, 3, 1, 1), row=good["row"].cpu()),
        "C = 257 with rows = -1": dict(attrs=z(3, 257), N=-1, grad_out=z(3)),
    })
    interp_backward = {"grad_out of another C": dict(grad_out=z(1, 4)), "grad_out on the CPU": dict(grad_out=th.zeros(1, 3))}
    k_values = lambda K: dict(face=iz(1, K, 1, 1), row=iz(1, K, 1, 1))
    values = _values_cases(z, good, k_values, lambda C: z(1, C))
    values.update(with_row)
    values.update({
        "values with one dimension": dict(values=z(3)),
        "empty fragment lists": dict(face=iz(1, 1, 0, 1), row=iz(1, 1, 0, 1)),
        "2^31 rows": dict(values=z(1, 1).expand(2 ** 31, 3)),
        "C = 257 with 2^31 rows": dict(values=z(1, 1).expand(2 ** 31, 257)),
    })
    values_backward = _values_backward_only(z)
    values_backward.update(n_used)  # (the forward call takes no n_used)
    return _refusals(good, [
        ("pack_slots", {"pack_slots": ("face", "F", "capacity")}, pack, {}),
        ("interpolate_packed", {"interpolate_packed": ("face", "bary", "row", "n_used", "faces", "attrs", "N"),
                                "interpolate_packed_backward": ("face", "bary", "row", "n_used", "faces", "attrs", "grad_out", "need2")},
         interp, interp_backward),
        ("composite_values_packed", {"composite_values_packed": ("face", "row", "opacity", "values", "scale"),
                                     "composite_values_packed_backward": ("face", "row", "n_used", "opacity", "values", "scale", "grad_image",
                                                                          "grad_T", "need3")},
         values, values_backward)])


LIST_REFUSALS = {"visibility": _visibility_refusals, "deferred": _deferred_refusals, "packed": _packed_refusals}
