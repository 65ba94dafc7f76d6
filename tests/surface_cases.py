"""The surface-frame unit (csrc/dmr_surface.hip: fragments.surface_packed_fused): the ctypes signatures of its two C calls, which
kernel instantiation a call reaches, and the list makers and case tables of tests/test_surface_gpu.py.  No GPU code: the GPU tests
import the tables from here, and tests/test_surface_cpu.py checks, without a GPU, the conditions on the inputs that the tables must
meet (the share of rows whose normal may flip between float32 and float64, no face near degenerate where none is meant).  In
packed_cases.py's and sh_cases.py's role.
"""
import ctypes as C
import functools
from collections import namedtuple

import torch as th

from dmesh_renderer_amd import Fragments
from dmesh_renderer_amd import fragments as FG
from shading_cases import EDGE_FRAMES, NEW_FRAME, SIZES

SOURCE, HEADER = "dmr_surface.hip", "dmesh_renderer_amd_surface.h"
FUNCTIONS = ["dmr_surface_packed", "dmr_surface_packed_backward"]
# name -> (leading ints, pointers with the trailing stream): row_units.SIGNATURES' form, for the calls that table does not hold
SIGNATURES = {"dmr_surface_packed": (7, 11), "dmr_surface_packed_backward": (7, 14)}
INTS = "B K H W P F N"
PTRS = {"dmr_surface_packed": "face bary row n_used faces verts origin hit normal reflect",
        "dmr_surface_packed_backward": "face bary row n_used faces verts origin grad_hit grad_normal grad_reflect dL_dverts dL_dbary dL_dorigin"}
OUTPUTS, UPSTREAMS, GRADS = ("hit", "normal", "reflect"), ("grad_hit", "grad_normal", "grad_reflect"), ("verts", "bary", "origin")


def declare(lib):
    """Sets restype and argtypes of the unit's two calls (and of dmr_last_error) on a ctypes library -> lib."""
    for name, (ints, pointers) in SIGNATURES.items():
        f = getattr(lib, name)
        f.restype, f.argtypes = C.c_int, [C.c_int] * ints + [C.c_void_p] * pointers
    lib.dmr_last_error.restype = C.c_char_p
    return lib


def instantiation(want):
    """The backward kernel a call that wants the gradients `want` (a subset of GRADS) launches, None for none."""
    return ("k_surface_packed_backward", tuple(g in want for g in GRADS)) if want else None


def every_instantiation():
    subsets = [tuple(g for i, g in enumerate(GRADS) if m >> i & 1) for m in range(1, 8)]
    return {("k_surface_packed", ())} | {instantiation(s) for s in subsets}


# ---------------------------------------------------------------------------
# Lists.  Vertices in the unit box, camera centres 2 to 4 away from its middle, 15 % of the slots empty anywhere in a list and
# 10 % ids past F (packed_cases' fills), barycentrics inside the face.  NEAR: the rows whose float32 and float64 normals may
# choose opposite signs, |m . d| < NEAR, are left out of the comparison of `normal` and get no upstream of it.
# ---------------------------------------------------------------------------
NEAR, NEAR_SHARE, MIN_AREA = 1e-3, 0.02, 1e-3
Case = namedtuple("Case", "K size frame cap extra_f special")   # cap: None = the exact count, else count + cap rows; extra_f: packed for F + extra_f


def case(K, size, frame=NEW_FRAME, cap=None, extra_f=0, special=None):
    assert 1 <= K <= 32 and size in SIZES and special in (None, "degenerate", "bad_vertex", "at_origin")
    return Case(K, size, tuple(frame), cap, extra_f, special)


def _areas(faces, verts):
    p = verts.double()[faces.long()]
    return th.linalg.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]).norm(dim=1)


@functools.lru_cache(maxsize=None)
def lists(c):
    """The CPU tensors of a case (float32 / int32): face, bary, faces, verts, origin, packed (for F + extra_f faces), count,
    the three upstreams with NaN in every row no counting slot holds, and `near` bool [N]: the rows left out of `normal`."""
    B, H, W = c.frame
    F, P = SIZES[c.size]
    g = th.Generator().manual_seed(5000 * c.K + 11 * H + (F > 100) + 3 * B + (c.cap or 0) + 7 * c.extra_f + len(c.special or ""))
    face = th.randint(0, F, (B, c.K, H, W), generator=g, dtype=th.int32)
    r = th.rand(B, c.K, H, W, generator=g)
    face = th.where(r < 0.15, th.full_like(face, -1), face)
    face = th.where((r >= 0.15) & (r < 0.25), face + F + (face % 3) * 5, face)   # F, F + 5.., past the faces
    bu = th.rand(B, c.K, 1, H, W, generator=g) * 0.9 + 0.05
    bv = (1 - bu) * (th.rand(B, c.K, 1, H, W, generator=g) * 0.9 + 0.05)
    bary = th.cat([bu, bv], 2)
    verts = th.rand(P, 3, generator=g)
    faces = th.randint(0, P, (F, 3), generator=g, dtype=th.int32)
    meant = th.zeros(F, dtype=th.bool)   # the faces that are degenerate on purpose
    if c.special == "degenerate":        # face 1: two equal vertices; face 2: three collinear ones, exactly (v2 = 2 v1 - v0 in eighths)
        verts[:3] = th.tensor([[0.25, 0.5, 0.125], [0.5, 0.25, 0.375], [0.75, 0.0, 0.625]])
        faces[1], faces[2], meant[1:3] = th.tensor([4, 4, 7], dtype=th.int32), th.tensor([0, 1, 2], dtype=th.int32), True
    for _ in range(64):   # resample what is degenerate or nearly so: the yardstick is not to be dominated by 1 / a
        thin = (_areas(faces, verts) < MIN_AREA) & ~meant
        if not bool(thin.any()):
            break
        faces[thin] = th.randint(0, P, (int(thin.sum()), 3), generator=g, dtype=th.int32)
    assert float(_areas(faces, verts)[~meant].min()) >= MIN_AREA and float(_areas(faces, verts)[meant].sum()) == 0
    d = th.randn(B, 3, generator=g)
    origin = 0.5 + d / d.norm(dim=1, keepdim=True) * (2 + 2 * th.rand(B, 1, generator=g))
    if c.special == "bad_vertex":     # vertex ids outside [0, P)
        faces[2, 1], faces[3, 0], faces[5, 2] = P, -1, 2 ** 31 - 1
    if c.special == "at_origin":      # the first view's camera sits on a vertex, and a slot hits exactly there
        origin[0] = verts[faces[0, 1].long()]
        face[0, 0, 0, 0] = 0
        bary[0, 0, :, 0, 0] = th.tensor([1.0, 0.0])
    pack_f = F + c.extra_f
    used = (face >= 0) & (face < pack_f)
    count = int(used.sum())
    packed = FG.pack_slots(Fragments(face, None, None), pack_f, None if c.cap is None else max(count + c.cap, 0))
    N = packed.rows
    out = dict(face=face, bary=bary, faces=faces, verts=verts, origin=origin, packed=packed, count=count, pack_f=pack_f,
               capacity=None if c.cap is None else N)
    with th.no_grad():   # in float64: which rows count, and which lie within NEAR of s = 0
        s64 = FG.surface_packed(Fragments(face, bary.double(), None), packed, faces, verts.double(), origin.double())
        d64 = s64.reflect - 2 * (s64.reflect * s64.normal).sum(1, keepdim=True) * s64.normal    # (the mirror of the mirror: d)
    counting = (packed.row >= 0) & (packed.row < N) & (face >= 0) & (face < F)
    held = th.zeros(N, dtype=th.bool)
    held[packed.row[counting].long()] = True
    near = held & ((s64.normal * d64).sum(1).abs() < NEAR) & (s64.normal.abs().sum(1) > 0)
    ups = {k: th.randn(N, 3, generator=g) for k in UPSTREAMS}
    for k in UPSTREAMS:
        ups[k][~held] = float("nan")
    ups["grad_normal"][near] = 0.0
    out.update(ups, near=near, held=held)
    return out


# ---------------------------------------------------------------------------
# The tables (the smallest shapes at which each mechanism can go wrong)
# ---------------------------------------------------------------------------
SMALL, LARGE = "shared_keys", "table_overflow"   # F = 7 / P = 9: many lanes of a wave on one face; F = 6000 / P = 9000: the table refuses rows
THREE_VIEWS = (3, 17, 33)                        # distinct origins: a wrong view index shows
TABLE = [case(1, SMALL), case(5, SMALL), case(32, SMALL), case(5, LARGE), case(32, LARGE, THREE_VIEWS), case(5, SMALL, THREE_VIEWS),
         case(1, LARGE, THREE_VIEWS)] + [case(5, SMALL, f) for f in EDGE_FRAMES] + [case(5, LARGE, EDGE_FRAMES[0])]
CAPACITY = [case(5, SMALL, THREE_VIEWS, cap=c) for c in (-300, 0, 130)]   # capacity below, at and above the count
OTHER_F = case(5, SMALL, THREE_VIEWS, extra_f=4)                           # a `packed` made for a larger F
DEGENERATE = case(5, SMALL, special="degenerate")
BAD_VERTEX = case(5, SMALL, THREE_VIEWS, special="bad_vertex")
AT_ORIGIN = case(5, LARGE, special="at_origin")   # (LARGE: few faces share the vertex the camera sits on, whose rows all have s = 0)
SUBSETS = case(5, SMALL, THREE_VIEWS)             # every subset of wanted gradients and of arriving upstreams
MISALIGNED = case(5, LARGE, THREE_VIEWS)          # verts one float off a 16-byte boundary, between sentinels
GRAPH = case(5, LARGE, THREE_VIEWS)


def all_cases():
    return TABLE + CAPACITY + [OTHER_F, DEGENERATE, BAD_VERTEX, AT_ORIGIN, SUBSETS, MISALIGNED, GRAPH]
