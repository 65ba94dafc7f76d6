"""The refusals of the four shading entry points of the C ABI (include/dmesh_renderer_amd_shade.h, dmesh_renderer_amd_texture.h),
without a GPU: every check of the argument validation and of the backward calls' prologue runs before any HIP call, so the
calls are made through ctypes with pointers that are never dereferenced.  Every refusal is tripped alone, and pairs of wrong
arguments say which message wins: the first failing check decides it.  The expected return values and dmr_last_error() texts
are a record of the library before the two units' host code was merged (tests/golden/shading_refusals.json, "c_abi").
No call here has wholly valid arguments and an output to write: none reaches a memset or a launch."""
import ctypes as C
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shading_refusals.json")
D = C.c_void_p(16)  # non-null, never dereferenced on these paths
INT_MAX = 2 ** 31 - 1

# name -> (the int arguments, the pointer arguments, in the header's order)
CALLS = {
    "dmr_composite_fragments": ("B K H W P F C", "face bary faces faces_opacity vert_attrs face_scale image T stream"),
    "dmr_composite_fragments_backward": ("B K H W P F C", "face bary faces faces_opacity vert_attrs face_scale grad_image grad_T "
                                         "dL_dfaces_opacity dL_dvert_attrs dL_dface_scale dL_dbary stream"),
    "dmr_composite_texture": ("B K H W Pu F C Ht Wt wrap", "face bary uv_faces faces_opacity vert_uvs texture face_scale image T stream"),
    "dmr_composite_texture_backward": ("B K H W Pu F C Ht Wt wrap", "face bary uv_faces faces_opacity vert_uvs texture face_scale "
                                       "grad_image grad_T dL_dfaces_opacity dL_dvert_uvs dL_dtexture dL_dface_scale dL_dbary stream"),
}
# valid sizes; every pointer is D but face_scale, the gradient outputs and the stream (null)
SIZES = dict(B=1, K=1, H=1, W=1, P=3, Pu=3, F=1, C=3, Ht=2, Wt=2, wrap=0)
NULL_BY_DEFAULT = ("face_scale", "stream", "dL_dfaces_opacity", "dL_dvert_attrs", "dL_dvert_uvs", "dL_dtexture", "dL_dface_scale", "dL_dbary")

# case -> the arguments it changes (a name a call does not take is skipped for that call).  Every case must be refused, or,
# in a backward call without a gradient output, return 0 before anything is enqueued.
LISTS = {  # both units, forward and backward
    "B=0": dict(B=0), "H=0": dict(H=0), "W=0": dict(W=0), "P<0": dict(P=-1, Pu=-1), "F<0": dict(F=-1),
    "K=0": dict(K=0), "K=33": dict(K=33), "C=0": dict(C=0), "C=max+1": None,  # (per unit, below)
    "null face": dict(face=None), "null bary": dict(bary=None),
    "null corner table": dict(faces=None, uv_faces=None), "null faces_opacity": dict(faces_opacity=None),
    "null per-vertex table": dict(vert_attrs=None, vert_uvs=None),
    "tiles >= 2^31": dict(B=INT_MAX, H=17, W=17), "B F >= 2^31": dict(B=65536, F=65536),
    # two at once: the first check wins
    "bad K and bad C": dict(K=0, C=0), "bad C and null lists": dict(C=0, face=None, bary=None),
    "bad dimensions and bad K": dict(W=0, K=99), "null lists and null corner table": dict(bary=None, faces=None, uv_faces=None),
    "null corner table and too large": dict(faces=None, uv_faces=None, B=65536, F=65536),
    "null per-vertex table and too large": dict(vert_attrs=None, vert_uvs=None, B=65536, F=65536),
}
TEXTURE_ONLY = {
    "Ht=0": dict(Ht=0), "Wt=0": dict(Wt=0), "wrap=2": dict(wrap=2), "wrap=-1": dict(wrap=-1),
    "texels >= 2^32 - 1": dict(Ht=65536, Wt=65536), "texel chunks >= 2^32 - 1": dict(Ht=65536, Wt=32768, C=5),
    "null texture": dict(texture=None),
    "bad C and bad wrap": dict(C=33, wrap=2), "bad Ht and bad wrap": dict(Ht=0, wrap=7), "bad wrap and null lists": dict(wrap=2, face=None),
    "texture too large and null lists": dict(Ht=65536, Wt=65536, face=None), "null vert_uvs and null texture": dict(vert_uvs=None, texture=None),
}
FORWARD_ONLY = {  # (the checks passed: a null output is the last refusal before the launch)
    "null image": dict(image=None), "null T": dict(T=None),
    "no faces, no corner table, null image": dict(F=0, faces=None, uv_faces=None, faces_opacity=None, image=None),
    "no vertices, no per-vertex table, null image": dict(P=0, Pu=0, vert_attrs=None, vert_uvs=None, image=None),
}
BACKWARD_ONLY = {
    "dL_dface_scale without face_scale": dict(dL_dface_scale=D),
    "no gradient wanted": dict(),  # returns 0
    "no gradient wanted, no upstream": dict(grad_image=None, grad_T=None),  # returns 0
    "bad K although no gradient wanted": dict(K=0),
}


def cases():
    """[(case id, call, {argument: value})]"""
    out = []
    for call, (ints, ptrs) in CALLS.items():
        texture, backward = "texture" in call, call.endswith("_backward")
        table = dict(LISTS)
        table["C=max+1"] = dict(C=33 if texture else 257)
        table.update(TEXTURE_ONLY if texture else {})
        table.update(BACKWARD_ONLY if backward else FORWARD_ONLY)
        for case, changes in table.items():
            out.append((f"{call}: {case}", call, {k: v for k, v in changes.items() if k in ints.split() + ptrs.split()}))
    return out


def library():
    import capi_ctypes
    lib = capi_ctypes.load()
    for call, (ints, ptrs) in CALLS.items():
        fn = getattr(lib, call)
        fn.restype = C.c_int
        fn.argtypes = [C.c_int] * len(ints.split()) + [C.c_void_p] * len(ptrs.split())
    return lib


def observe(lib, call, changes):
    """(return value, dmr_last_error() after a non-zero one)"""
    ints, ptrs = CALLS[call]
    args = [changes.get(n, SIZES[n]) for n in ints.split()]
    args += [changes.get(n, None if n in NULL_BY_DEFAULT else D) for n in ptrs.split()]
    ret = getattr(lib, call)(*args)
    return [ret, lib.dmr_last_error().decode() if ret else ""]


def observed():
    lib = library()
    return {cid: observe(lib, call, changes) for cid, call, changes in cases()}


@pytest.fixture(scope="module")
def golden():
    return json.load(open(GOLDEN))["c_abi"]


def test_the_record_covers_the_cases(golden):
    assert sorted(golden) == sorted(cid for cid, _, _ in cases())
    # every message of the two validations and the prologues is tripped, in all four calls where it applies
    texts = {m.split(": ", 1)[1] for _, m in golden.values() if m}
    for part in ("bad dimensions", "K must be in 1..32, got 0", "K must be in 1..32, got 33", "C must be in 1..256, got 257",
                 "C must be in 1..32, got 33", "null fragment lists", "null faces / faces_opacity", "null uv_faces / faces_opacity",
                 "null vert_attrs", "null vert_uvs", "null texture", "problem too large", "null output",
                 "the texture must have at least one texel", "wrap must be 0 (clamp) or 1 (repeat), got 2",
                 "texture too large: Ht * Wt * ceil(C / 4) must be below 2^32 - 1", "dL_dface_scale without face_scale"):
        assert part in texts, part
    assert sum(1 for r, _ in golden.values() if r == 0) == 4  # the two backward calls, with and without an upstream


def test_every_refusal_and_its_text(golden):
    got = observed()
    for cid, _, _ in cases():
        assert got[cid] == golden[cid], cid


def test_the_first_failing_check_decides(golden):
    """The pairs, spelt out: what wins is the check that comes first in the call."""
    got = observed()
    for call in CALLS:
        n = call + ": "
        cmax = 32 if "texture" in call else 256
        assert got[n + "bad K and bad C"] == [1, n + "K must be in 1..32, got 0"]
        assert got[n + "bad C and null lists"] == [1, n + f"C must be in 1..{cmax}, got 0"]
        assert got[n + "bad dimensions and bad K"] == [1, n + "bad dimensions"]
        assert got[n + "null lists and null corner table"] == [1, n + "null fragment lists"]
        assert got[n + "null corner table and too large"][1].startswith(n + "null ")
        assert got[n + "null per-vertex table and too large"][1].startswith(n + "null vert_")
        if "texture" in call:
            assert got[n + "bad C and bad wrap"] == [1, n + "C must be in 1..32, got 33"]
            assert got[n + "bad Ht and bad wrap"] == [1, n + "the texture must have at least one texel"]
            assert got[n + "bad wrap and null lists"] == [1, n + "wrap must be 0 (clamp) or 1 (repeat), got 2"]
            assert got[n + "texture too large and null lists"][1].startswith(n + "texture too large")
            assert got[n + "null vert_uvs and null texture"] == [1, n + "null vert_uvs"]
        if call.endswith("_backward"):
            assert got[n + "no gradient wanted"] == [0, ""] and got[n + "no gradient wanted, no upstream"] == [0, ""]
            assert got[n + "bad K although no gradient wanted"] == [1, n + "K must be in 1..32, got 0"]
