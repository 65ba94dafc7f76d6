"""dmesh_renderer_amd -- MI355X-native drop-in for the hot path of SonSang/dmesh_renderer.

Public surface = the reference package's (dmesh_renderer/__init__.py):
    TriRenderSettings, render_tri, TriRenderer      (:13-16, :18-43, :172-225)
    TetRenderSettings, render_tet, TetRenderer      (:237-241, :243-275, :426-488)
with identical argument order, dtypes, shapes, outputs and gradient routing.  The compute
lives in libdmesh_renderer_hip.so (hand-written gfx950 kernels) behind `_C`.

Conventions kept from the reference: the Modules receive ROW-major [B,4,4] matrices and
pass transposed views down (:219-220, :476-477); _TriFn / _TetFn invert those
(:62-63, :298-299); the tri Module only casts `faces`, the tet Module casts everything (Q23).
"""
from __future__ import annotations

import math
from operator import itemgetter
from typing import List, NamedTuple, Optional, Tuple

import torch as th

class _NotBuilt:
    """Stands in for `_C` while the native pieces are missing, so that `dmesh_renderer_amd.build` itself stays
    importable; any use of the renderer raises -- there is no CPU or Python fallback."""

    def __init__(self, cause):
        self._cause = cause

    def __getattr__(self, name):
        raise ImportError(f"dmesh_renderer_amd._C cannot be imported ({self._cause}). Build the native pieces first: "
                          "`python -m dmesh_renderer_amd.build` (hipcc + g++, in-tree); there is no CPU or Python fallback.")


try:
    from . import _C  # the compiled binding (csrc/dmr_torch.cpp) over libdmesh_renderer_hip.so
except ImportError as _e:  # not built yet, or its HIP library is missing / of another ABI version
    _C = _NotBuilt(_e)

__all__ = ["TriRenderSettings", "render_tri", "TriRenderer", "TetRenderSettings", "render_tet", "TetRenderer", "Fragments"]


class TriRenderSettings(NamedTuple):
    image_height: int
    image_width: int
    bg: th.Tensor


class TetRenderSettings(NamedTuple):
    image_height: int
    image_width: int
    bg: th.Tensor
    ray_random_seed: int


def _with_inverses(mv_mats: th.Tensor, proj_mats: th.Tensor) -> Tuple[th.Tensor, ...]:
    """(mv, proj, mv^-1, proj^-1), reference :62-63.  On a HIP device the two inverses come from one library kernel
    (_C.invert_mats) instead of two th.inverse calls; anything else (CPU tensors in the wrapper tests, other
    dtypes) takes th.inverse like the reference."""
    if mv_mats.is_cuda and proj_mats.is_cuda and mv_mats.dtype == th.float32 and proj_mats.dtype == th.float32 \
            and mv_mats.dim() == 3 and proj_mats.dim() == 3:
        return (mv_mats, proj_mats) + _C.invert_mats(mv_mats, proj_mats)
    return mv_mats, proj_mats, th.inverse(mv_mats), th.inverse(proj_mats)


def _through_inverse(y: th.Tensor, g: th.Tensor) -> th.Tensor:
    """dL/dX from g = dL/dY for Y = X^-1 ([B,4,4] each): -Y^T g Y^T."""
    yt = y.transpose(1, 2)
    return -th.matmul(th.matmul(yt, g), yt)


def _trailing(*args) -> tuple:
    """The optional trailing arguments of _TriFn / _TetFn.apply without the unset ones at the end: every argument of
    apply costs host time on each call, and the default call passes none."""
    n = len(args)
    while n and not args[n - 1]:
        n -= 1
    return args[:n]


def _alpha_kw(alpha) -> dict:
    """The `alpha` keyword of the four `_C` functions; no keyword by default: the reference's call."""
    return {"alpha": True} if alpha else {}


class Fragments(NamedTuple):
    """Per-pixel fragment lists of either renderer (return_fragments=K; helpers in dmesh_renderer_amd.fragments): the faces each
    pixel blended, front to back, and where its ray hit them.  Constants of every gradient, like coverage and list order --
    unless the TRI renderer was made with fragment_grads=True: `bary` then takes part in autograd (its gradient reaches verts
    and, with camera_grads, the matrices); pix_to_face and count stay constants.  The tet renderer's lists are in exact march
    order, their barycentrics unclamped (a face the march crosses is hit in its interior); TetRenderer(fragment_grads=True)
    makes its `bary` differentiable in the same way (there is no clamp, so no clamp region; the option implies full_grads)."""
    pix_to_face: th.Tensor  # int32 [B,K,H,W]: face ids in blend order, -1 in unused slots
    bary: th.Tensor         # float32 [B,K,2,H,W]: (u, v), clamped by the tri renderer; the weights of the face's vertices are (1 - u - v, u, v)
    count: th.Tensor        # int32 [B,H,W]: blended faces of the pixel (tet: 0 where the march failed); above K the list is truncated to its first K


def _split_fragments(out, alpha):
    """(color, depth, face, bary, count) of _TriFn / (color, depth, active, face, bary, count) of _TetFn called with fragments
    -> (color, depth[, active][, alpha], Fragments)."""
    head = _split_alpha(out[:-3]) if alpha else tuple(out[:-3])
    return (*head, Fragments(*out[-3:]))


def _split_alpha(out):
    """(color, depth | alpha [B,2,H,W], ...) of a Function called with alpha -> (color, depth, ..., alpha [B,1,H,W]).  Slices
    of one tensor: autograd assembles the two-channel upstream gradient (zeros for a channel the loss does not use)."""
    return (out[0], out[1][:, :1], *out[2:], out[1][:, 1:])


def _outputs(out, alpha, fragments):
    """What a Function returned -> what render_tri / render_tet and the Modules return."""
    if fragments:
        return _split_fragments(out, alpha)
    return _split_alpha(out) if alpha else out


def _fragment_kw(fragments, fragment_grads, shard) -> dict:
    """The option checks of _TriFn / _TetFn and the `fragments` keyword of their _forward (none by default)."""
    if fragment_grads and shard is not None:
        raise ValueError("fragment_grads is not available on the sharded Modules")
    if fragments and shard is not None:
        raise ValueError("return_fragments is not available on the sharded Modules")
    if fragment_grads and not fragments:
        raise ValueError("fragment_grads needs return_fragments=K: it is the gradient of the fragment lists' barycentrics")
    return {"fragments": fragments} if fragments else {}


def _save(ctx, saved, fragment_grads, color, depth, frag, constants=()):
    """The end of _TriFn / _TetFn.forward: what the backward needs, and which outputs are constants (`constants` and the
    fragment lists -- but for bary with fragment_grads: face is then what the backward needs of the lists)."""
    ctx.fragment_grads = bool(fragment_grads)
    if fragment_grads:
        ctx.save_for_backward(*saved, frag[0])
        ctx.mark_non_differentiable(*constants, frag[0], frag[2])
        ctx.set_materialize_grads(False)  # no zeros for the outputs a loss does not use: a None for bary is the call without the term
        ctx.image_shapes = (color.shape, depth.shape)
    else:
        ctx.save_for_backward(*saved)
        ctx.mark_non_differentiable(*constants, *frag)


def _upstream(ctx, grad_color, grad_depth, grad_fragments):
    """The gradients autograd hands to _TriFn / _TetFn.backward -> (grad_color, grad_depth, further keywords of _backward).
    With fragment_grads the image gradients may be missing (zeros then), and one for bary goes down with the call."""
    more = {}
    if ctx.fragment_grads:
        more["extra_saved"] = 1  # (face)
        if grad_color is None:
            grad_color = ctx.saved_tensors[0].new_zeros(ctx.image_shapes[0])
        if grad_depth is None:
            grad_depth = ctx.saved_tensors[0].new_zeros(ctx.image_shapes[1])
        if grad_fragments[1] is not None:
            more["fragment_grads"] = (ctx.saved_tensors[-1], grad_fragments[1].contiguous())
    return grad_color, grad_depth, more


def _impl(shard):
    """The kernels of a Function: `_C` as it is at call time on one device (tests swap it), a sharded Module's otherwise."""
    return _C if shard is None else shard.impl


def _forward(render, settings, geom, mv_mats, proj_mats, verts_depth, faces_intense, rows, alpha=False, topo=(), **more):
    """One render_tris / render_tets (with topo) call -> (its three results: num_rendered, color, depth / color, depth,
    active -- followed by what `more`, further keywords of the call, adds behind the scratch buffers; what its backward needs
    after geom: the matrices, their inverses, verts_depth, faces_intense, topo and the four scratch buffers).  alpha: depth is
    [B,2,H,W], depth | alpha."""
    cams = _with_inverses(mv_mats, proj_mats)
    try:  # (settings[3:]: the tet settings' ray_random_seed)
        out = render(settings.bg, *geom, *cams, verts_depth, faces_intense, *topo, settings.image_height, settings.image_width,
                     *settings[3:], rows=rows, **_alpha_kw(alpha), **more)
    except Exception as ex:
        print("\nAn error occured in forward.")
        if not topo:  # (as the reference: its tri wrapper prints the exception, its tet wrapper does not)
            print(ex)
        raise
    return (*out[:3], *out[7:]), (*cams, verts_depth, faces_intense, *topo, *out[3:7])


def _one_backward(render_backward, settings, geom, saved, upstream, rows, kw):
    """One render_tris_backward / render_tets_backward call for a _forward: upstream = (grad_color, grad_depth) and, tri,
    num_rendered."""
    try:
        return render_backward(settings.bg, *geom, *saved[:-4], *upstream, *saved[-4:], rows=rows, **kw)
    except Exception:
        print("\nAn error occured in backward.\n")
        raise


class _GradSet:
    """The gradient set of one renderer, stated once for _TriFn, _TetFn and sharding._ShardedTriViewFn.  (GradTable in
    csrc/dmr_torch.cpp states the same for `_C`; the two meet in flat_out, whose size the binding checks.)  A backward has a
    level: 0 the reference's gradients, 1 exact_grads (tri) / full_grads (tet), 2 camera_grads, which implies level 1.
    backward: its name in `_C`; level_kw: its keyword of level 1.
    shapes: (P, F, B) -> the shapes of the pieces of the flat buffer (what flat_out= receives, the payload of the one all-reduce),
    in its order; the last is the camera piece, [B, n, 4, 4]: n matrix gradients per view.
    order: per level, the pieces it holds but the camera one (level 2 only) in the order of the backward's tuple; the camera
    piece's n [B,4,4] slices follow.
    inputs: per piece but the camera one, the argument of apply it is the gradient of (the camera piece reaches arguments 4 and
    5, mv_mats and proj_mats, through _camera_grads).
    pick: per level, (*that tuple's gradients, dL/dmv, dL/dproj, None) -> the gradients of apply's eight tensors."""

    def __init__(self, backward: str, level_kw: str, shapes, inputs, order):
        self.backward, self.level_kw, self.shapes, self.order, self.pick = backward, level_kw, shapes, order, []
        for o in order:
            at = [len(o) + 2] * 8  # None
            at[4], at[5] = len(o), len(o) + 1
            for k, piece in enumerate(o):
                at[inputs[piece]] = k
            self.pick.append(itemgetter(*at))


# [3P | 3P | F | BP | BF], with camera grads followed by [B][dL/dinv_mv 16 | dL/dinv_proj 16]
_TRI_GRADS = _GradSet("render_tris_backward", "exact_grads", lambda P, F, B: ((P, 3), (P, 3), (F,), (B, P), (B, F), (B, 2, 4, 4)),
                      inputs=(0, 2, 3, 6, 7), order=((0, 1, 2, 3, 4),) * 3)
# [dL_dverts_color 3P | dL_dfaces_opacity F], with full_grads followed by [dL_dverts 3P | dL_dfaces_intense BF], with camera
# grads then by [B][dL/dinv_mv 16 | dL/dinv_proj 16 | dL/dmv 16 | dL/dproj 16]
_TET_GRADS = _GradSet("render_tets_backward", "full_grads", lambda P, F, B: ((P, 3), (F,), (P, 3), (B, F), (B, 4, 4, 4)),
                      inputs=(2, 3, 0, 7), order=((0, 1), (2, 0, 1, 3), (2, 0, 1, 3)))


def _grad_options(ctx, gs: _GradSet) -> Tuple[int, dict]:
    """(level, keywords of the backward).  The matrices' gradients are computed only when asked for and a matrix needs one:
    otherwise level 1, which skips the per-pixel ray sums.  No keyword by default: the reference's call.  (A fresh dict: the
    caller may add flat_out.)  With ctx.alpha also alpha=True: grad_depth is [B,2,H,W]."""
    if ctx.camera_grads and (ctx.needs_input_grad[4] or ctx.needs_input_grad[5]):
        return 2, {"camera_grads": True, **_alpha_kw(ctx.alpha)}
    return int(ctx.more_grads), {**({gs.level_kw: True} if ctx.more_grads else {}), **_alpha_kw(ctx.alpha)}


def _flat(gs: _GradSet, level: int, P: int, F: int, B: int, device, alloc=th.empty) -> Tuple[th.Tensor, List[th.Tensor]]:
    """The flat gradient buffer of a backward (what flat_out= fills) and its pieces as views of their shapes."""
    shapes = gs.shapes(P, F, B)
    shapes = shapes[:len(gs.order[level])] + shapes[-1:] * (level == 2)
    sizes = [math.prod(s) for s in shapes]
    flat = alloc(sum(sizes), dtype=th.float32, device=device)
    return flat, [p.view(s) for p, s in zip(flat.split(sizes), shapes)]


def _camera_grads(ctx, inv_mv, inv_proj, g_inv_mv, g_inv_proj, g_mv=None,
                  g_proj=None) -> Tuple[Optional[th.Tensor], Optional[th.Tensor]]:
    """dL/d(inverse) -> dL/d(matrix) for the matrices (inputs 4 and 5) that need a gradient, plus the direct terms g_mv,
    g_proj of a renderer that also reads the matrices themselves (the tet renderer's depth)."""
    def one(i, inv, g_inv, direct):
        if not ctx.needs_input_grad[i]:
            return None
        g = _through_inverse(inv, g_inv)
        return g if direct is None else direct + g
    return one(4, inv_mv, g_inv_mv, g_mv), one(5, inv_proj, g_inv_proj, g_proj)


def _input_grads(ctx, gs: _GradSet, level: int, g, inv_mv, inv_proj) -> tuple:
    """A backward's tuple `g` -> the gradients of apply's eight tensors (None where there is none)."""
    k = len(gs.order[level])
    mats = _camera_grads(ctx, inv_mv, inv_proj, *g[k:]) if level == 2 else (None, None)
    return gs.pick[level]((*g[:k], *mats, None))


def _backward(ctx, gs: _GradSet, *upstream, extra_saved=0, **more) -> tuple:
    """The backward of _TriFn / _TetFn: one _one_backward at ctx's level, the all-reduce of a sharded Module, the gradients of
    apply's eight tensors.  more: further keywords of the call (fragment_grads of either Function) whose terms the library adds into
    pieces of the level's gradient set: nothing new in the tuple.  extra_saved: tensors the Function saved behind _forward's."""
    saved = ctx.saved_tensors
    geom, saved = saved[:4], saved[4:len(saved) - extra_saved]
    level, kw = _grad_options(ctx, gs)
    kw.update(more)
    shard, flat = ctx.shard, None
    if shard is not None and shard.flat_out:  # the gradients land back to back in the all-reduce payload
        flat = kw["flat_out"] = _flat(gs, level, geom[0].size(0), geom[1].size(0), saved[0].size(0), geom[0].device)[0]
    g = _one_backward(getattr(_impl(shard), gs.backward), ctx.settings, geom, saved, upstream, ctx.rows, kw)
    if shard is not None:
        g = shard.reduce(g, flat)
    return _input_grads(ctx, gs, level, g, saved[2], saved[3])


class _TriFn(th.autograd.Function):
    """Inputs: verts, faces, verts_color, faces_opacity, mv^T, proj^T, verts_depth, faces_intense, settings, rows, shard,
    exact_grads, camera_grads, alpha, fragments, fragment_grads (the last six only when set: see _trailing).  Gradients flow to verts, verts_color,
    faces_opacity, verts_depth, faces_intense; with camera_grads also to mv^T and proj^T (see TriRenderer).  alpha: the
    second output is [B,2,H,W], depth | alpha (the caller slices it: _split_alpha), and so is its gradient.  shard: None
    on one device; from a sharded Module (sharding._Shard) its kernels, the band images to assemble and the gradients'
    all-reduce.  fragments = K > 0 (one device only): three more outputs, the non-differentiable face [B,K,H,W], bary
    [B,K,2,H,W] and count [B,H,W] of render_tris(fragments=K).  fragment_grads (needs fragments): bary is differentiable;
    the gradient that arrives for it goes down with the backward call (fragment_grads=(face, grad_bary): _upstream), where the
    library adds its term to the verts piece and, at level 2, to the inverse matrices' part of the camera piece: the gradient
    set is unchanged.  Gradients are then not materialised: a backward without one for bary is the call without the keyword."""

    @staticmethod
    def forward(ctx, verts, faces, verts_color, faces_opacity, mv_mats, proj_mats, verts_depth, faces_intense,
                settings: TriRenderSettings, rows, shard=None, exact_grads=False, camera_grads=False, alpha=False, fragments=0,
                fragment_grads=False):
        geom = (verts, faces, verts_color, faces_opacity)
        kw = _fragment_kw(fragments, fragment_grads, shard)
        (num_rendered, color, depth, *frag), saved = _forward(_impl(shard).render_tris, settings, geom, mv_mats, proj_mats, verts_depth,
                                                              faces_intense, rows, alpha, **kw)
        if shard is not None:
            color, depth = shard.gather((color, depth))
        ctx.settings, ctx.rows, ctx.shard, ctx.num_rendered = settings, rows, shard, num_rendered
        ctx.more_grads, ctx.camera_grads, ctx.alpha = exact_grads or camera_grads, camera_grads, alpha
        _save(ctx, (*geom, *saved), fragment_grads, color, depth, frag)
        return (color, depth, *frag)

    @staticmethod
    def backward(ctx, grad_color, grad_depth, *grad_fragments):
        grad_color, grad_depth, more = _upstream(ctx, grad_color, grad_depth, grad_fragments)
        return _backward(ctx, _TRI_GRADS, grad_color, grad_depth, ctx.num_rendered, **more) + (None,) * 8


class _TetFn(th.autograd.Function):
    """Gradients flow to verts_color and faces_opacity only (reference :407-422); with full_grads also to verts and
    faces_intense, with camera_grads also to mv^T and proj^T (beyond the reference).  shard, alpha, fragments (the lists of
    render_tets(fragments=K)) and fragment_grads (the last argument): as for _TriFn; fragment_grads implies full_grads, where
    dL/dverts exists, so a backward without a gradient for bary is the full_grads call."""

    @staticmethod
    def forward(ctx, verts, faces, verts_color, faces_opacity, mv_mats, proj_mats, verts_depth, faces_intense,
                tets, face_tets, tet_faces, settings: TetRenderSettings, rows, shard=None, full_grads=False, camera_grads=False,
                alpha=False, fragments=0, fragment_grads=False):
        geom = (verts, faces, verts_color, faces_opacity)
        kw = _fragment_kw(fragments, fragment_grads, shard)
        (color, depth, active, *frag), saved = _forward(_impl(shard).render_tets, settings, geom, mv_mats, proj_mats, verts_depth,
                                                        faces_intense, rows, alpha, (tets, face_tets, tet_faces), **kw)
        if shard is not None:
            color, depth, active = shard.gather((color, depth, active))
        active = active > 0.5  # bool mask, reference :333
        ctx.settings, ctx.rows, ctx.shard = settings, rows, shard
        ctx.more_grads, ctx.camera_grads, ctx.alpha = full_grads or camera_grads or bool(fragment_grads), camera_grads, alpha
        _save(ctx, (*geom, *saved), fragment_grads, color, depth, frag, constants=(active,))
        return (color, depth, active, *frag)

    @staticmethod
    def backward(ctx, grad_color, grad_depth, _grad_active, *grad_fragments):
        grad_color, grad_depth, more = _upstream(ctx, grad_color, grad_depth, grad_fragments)
        return _backward(ctx, _TET_GRADS, grad_color, grad_depth, **more) + (None,) * 11


def _check_fragment_grads(fragment_grads, return_fragments, tet=False):
    """The options of render_tri / render_tet and the Modules.  tet: the binding in use must also know render_tets_backward's
    fragment_grads keyword.  The binding is a build product of its own (build.py rebuilds it by file times): one from before
    the keyword, or a stand-in without it, would fail with pybind's argument dump in the first backward that carries a gradient
    for bary -- deep inside autograd.  Asked at construction instead, a TypeError that says what is missing."""
    if fragment_grads and not return_fragments:
        raise ValueError("fragment_grads=True needs return_fragments=K: it is the gradient of the fragment lists' barycentrics")
    if tet and fragment_grads and not getattr(_C, "SUPPORTS_TET_FRAGMENT_GRADS", False):
        raise TypeError("fragment_grads=True: the loaded binding's render_tets_backward has no fragment_grads keyword "
                        "(a `_C` built before it: rebuild with `python -m dmesh_renderer_amd.build --force`)")


def render_tri(verts, faces, verts_color, faces_opacity, mv_mats, proj_mats, verts_depth, faces_intense,
               render_settings: TriRenderSettings, rows=(0, 0), exact_grads=False, camera_grads=False, return_alpha=False,
               return_fragments=0, fragment_grads=False):
    """Functional form (reference :18-43).  mv_mats / proj_mats are the TRANSPOSED matrices.  exact_grads,
    camera_grads, return_alpha, return_fragments, fragment_grads: see TriRenderer."""
    _check_fragment_grads(fragment_grads, return_fragments)
    out = _TriFn.apply(verts, faces, verts_color, faces_opacity, mv_mats, proj_mats, verts_depth, faces_intense,
                       render_settings, tuple(rows),
                       *_trailing(None, bool(exact_grads), bool(camera_grads), bool(return_alpha), int(return_fragments),
                                  bool(fragment_grads)))
    return _outputs(out, return_alpha, return_fragments)


def render_tet(verts, faces, verts_color, faces_opacity, mv_mats, proj_mats, verts_depth, faces_intense,
               tets, face_tets, tet_faces, render_settings: TetRenderSettings, rows=(0, 0), full_grads=False, camera_grads=False,
               return_alpha=False, return_fragments=0, fragment_grads=False):
    """Functional form (reference :243-275).  mv_mats / proj_mats are the TRANSPOSED matrices.  full_grads,
    camera_grads, return_alpha, return_fragments, fragment_grads: see TetRenderer."""
    _check_fragment_grads(fragment_grads, return_fragments, tet=True)
    out = _TetFn.apply(verts, faces, verts_color, faces_opacity, mv_mats, proj_mats, verts_depth, faces_intense,
                       tets, face_tets, tet_faces, render_settings, tuple(rows),
                       *_trailing(None, bool(full_grads), bool(camera_grads), bool(return_alpha), int(return_fragments),
                                  bool(fragment_grads)))
    return _outputs(out, return_alpha, return_fragments)


class TriRenderer(th.nn.Module):
    """Renderer for (semi-transparent) triangles: depth-sorted front-to-back compositing of every
    triangle of a tile; no exact per-pixel depth test (reference README.md:3).

    exact_grads=True (beyond the reference): verts receive the true derivative of color and depth.  Each blended
    (pixel, face) pair enters through the Moeller-Trumbore (u, v) of the pixel's ray on the face, and that (u, v) is
    differentiated exactly.  The reference's gradient, the default, differentiates t where it means v.
    Coverage, list order and the clamp region of (u, v) are constants of the gradient, as for every gradient here.
    The other gradients are the default's, summed in another order.

    camera_grads=True (implies exact_grads): mv_mats and proj_mats receive gradients too, through every pixel's ray
    (its origin and direction come from the inverse matrices).  The depth output reads verts_depth, not the
    matrices: a caller who computes verts_depth from the camera gets that part through their own autograd.

    Both options cost a slower backward; the forward is the same.

    return_alpha=True (beyond the reference): a third image, alpha [B,1,H,W] = 1 - T, the accumulated opacity (coverage)
    of the pixel, T being the transmittance the renderer multiplies into the background: color == C + (1 - alpha) * bg.
    0 where nothing was blended and outside a rendered row band.  Its gradient reaches faces_opacity only
    (d alpha / d opacity_i = T / (1 - opacity_i) for every blended face) and combines with the options above: a mask
    loss, or a per-pixel background composited in torch -- render with bg = 0, then color + (1 - alpha) * bg_image.

    return_fragments=K, 1 <= K <= 32 (beyond the reference): the last output is a Fragments tuple (pix_to_face int32
    [B,K,H,W], bary float32 [B,K,2,H,W], count int32 [B,H,W]): per pixel the first K faces it blended, front to back, the
    clamped barycentrics its ray hit them at, and how many it blended in all (count > K: the list is truncated).  What a
    general rasteriser hands to a shader: dmesh_renderer_amd.fragments rebuilds blend weights, interpolates any per-vertex
    attribute, composites and sums per-face visibility from them in plain, differentiable torch.  The three tensors are
    constants (no gradient flows into them); the images and the backward are those of a call without the option.  One
    device only: the sharded Modules do not take it.

    fragment_grads=True (only with return_fragments=K): Fragments.bary takes part in autograd.  The gradient a loss sends
    into it -- through fragments.interpolate / composite, or any torch code that reads bary -- reaches verts as the exact
    derivative of the clamped Moeller-Trumbore (u_c, v_c) of each stored (pixel, face) pair, whatever exact_grads says about
    the images' own gradient, and with camera_grads (when a matrix needs a gradient) mv_mats and proj_mats through the
    pixel's ray.  Coverage, list order and the clamp region are constants, as for every gradient here; pix_to_face and
    count stay non-differentiable; pairs beyond K are not stored and get nothing.  One more kernel in the backward when a
    gradient for bary arrives; the forward and a backward without one are unchanged.

    forward(verts [P,3], faces [F,3], verts_color [P,3], faces_opacity [F],
            mv_mats [B,4,4], proj_mats [B,4,4], verts_depth [B,P], faces_intense [B,F])
        -> color [B,3,H,W], depth [B,1,H,W] (, alpha [B,1,H,W] with return_alpha) (, Fragments with return_fragments)
    """

    def __init__(self, render_settings: TriRenderSettings, exact_grads: bool = False, camera_grads: bool = False,
                 return_alpha: bool = False, return_fragments: int = 0, fragment_grads: bool = False):
        super().__init__()
        _check_fragment_grads(fragment_grads, return_fragments)
        self.render_settings = render_settings
        self.exact_grads = bool(exact_grads)
        self.camera_grads = bool(camera_grads)
        self.return_alpha = bool(return_alpha)
        self.return_fragments = int(return_fragments)
        self.fragment_grads = bool(fragment_grads)

    def forward(self, verts, faces, verts_color, faces_opacity, mv_mats, proj_mats, verts_depth, faces_intense):
        out = self._render(verts, faces.to(dtype=th.int32), verts_color, faces_opacity,
                           mv_mats.transpose(1, 2), proj_mats.transpose(1, 2), verts_depth, faces_intense)
        return _outputs(out, self.return_alpha, self.return_fragments)

    def _render(self, *inputs):
        """_TriFn on the normalised inputs (faces int32, the matrices transposed); ShardedTriRenderer adds a partition."""
        rows, shard = self._shard()
        return _TriFn.apply(*inputs, self.render_settings, rows,
                            *_trailing(shard, self.exact_grads, self.camera_grads, self.return_alpha, self.return_fragments,
                                       self.fragment_grads))

    def _shard(self):
        """(rows, shard) of the Functions: all rows on one device (the sharded Modules return their band)."""
        return (0, 0), None


class TetRenderer(th.nn.Module):
    """Renderer for the faces of a compact set of tetrahedra: the ray is marched tet to tet, so
    faces are composited in exact depth order; gradients reach verts_color and faces_opacity only
    (reference README.md:4).

    full_grads=True (beyond the reference, which has no such gradients): gradients also reach verts and
    faces_intense.  On the forward's march each composited face enters through the ray's hit (t, u, v) on it: u, v
    set its interpolated colour, t the hit point and so its ndc depth; the march itself (which faces, in which order)
    and the opacities are constants of the gradient.  verts_depth (not read by this renderer) gets none.

    camera_grads=True (implies full_grads): mv_mats and proj_mats receive gradients too.  Every pixel's ray (origin
    and direction from the inverse matrices) moves each composited face's hit, and the depth output reads the
    matrices directly through each hit point's ndc depth.  The seeded jitter of the ray is a constant of the gradient.

    Both options cost a slower backward; the forward is the same.

    return_alpha=True (beyond the reference): a fourth output, alpha [B,1,H,W] = 1 - T as TriRenderer's; 0 where the
    march fails (active == False: the colour there is the bare background).  Its gradient reaches faces_opacity only.

    return_fragments=K, 1 <= K <= 32 (beyond the reference): the last output is a Fragments tuple (pix_to_face int32
    [B,K,H,W], bary float32 [B,K,2,H,W], count int32 [B,H,W]), as TriRenderer's, here in EXACT march order: per pixel the
    first K faces its ray composited, front to back, the unclamped (u, v) it hit them at (a tet hit is interior by
    construction), and the number of its march steps (count > K: the list is truncated).  A pixel whose march fails
    (active == False) has count 0 and no fragments, whatever it crossed: its colour is the bare background.
    dmesh_renderer_amd.fragments shades from them -- normals, positions (interpolate(frag, faces, verts) is the hit point),
    feature channels, texture coordinates, per-face visibility -- in plain torch: composite(...) + T * bg is this renderer's
    colour where count <= K, except that behind a face of opacity 1 the renderer goes on with T = 1e-5 (T_EPS / 10), not 0.
    The three tensors are constants (no gradient flows into them) unless fragment_grads is set; the images and the
    backward are those of a call without the option.  One device only: the sharded Modules do not take it.

    fragment_grads=True (only with return_fragments=K; IMPLIES full_grads, the level at which this renderer has a gradient
    for verts at all: with the option the images' own gradient reaches verts and faces_intense as well): Fragments.bary
    takes part in autograd.  The gradient a loss sends into it -- through fragments.interpolate / composite, or any torch
    code that reads bary -- reaches verts as the exact derivative of the unclamped Moeller-Trumbore (u, v) of each stored
    (pixel, face) pair on the pixel's ray, and with camera_grads (when a matrix needs a gradient) mv_mats and proj_mats
    through that ray (origin and direction come from the inverse matrices; (u, v) do not read the matrices themselves).
    So the gradient of fragments.interpolate(frag, faces, verts) to verts is the full derivative of the hit point, the
    direct term through the vertex rows plus the movement of (u, v).  Which faces the march crossed, their order and the
    seeded jitter are constants; there is no clamp and so no clamp region; pix_to_face and count stay non-differentiable;
    pairs beyond K are not stored and get nothing.  One more kernel in the backward when a gradient for bary arrives
    (INTEGRATION.md); the forward is unchanged, and a backward without one is the full_grads call.  A binding that does not
    announce render_tets_backward's fragment_grads keyword (_C.SUPPORTS_TET_FRAGMENT_GRADS: a stale build of `_C`, or a
    stand-in for it) is a TypeError here, at construction, not in the first backward that would use it.

    forward(verts, faces, verts_color, faces_opacity, mv_mats, proj_mats, verts_depth, faces_intense,
            tets [T,4], face_tets [F,2] (-1 = none), tet_faces [T,4])
        -> color [B,3,H,W], depth [B,1,H,W], active bool [B,H,W] (, alpha [B,1,H,W] with return_alpha)
           (, Fragments with return_fragments)
    """

    def __init__(self, render_settings: TetRenderSettings, full_grads: bool = False, camera_grads: bool = False,
                 return_alpha: bool = False, return_fragments: int = 0, fragment_grads: bool = False):
        super().__init__()
        _check_fragment_grads(fragment_grads, return_fragments, tet=True)
        self.render_settings = render_settings
        self.full_grads = bool(full_grads)
        self.camera_grads = bool(camera_grads)
        self.return_alpha = bool(return_alpha)
        self.return_fragments = int(return_fragments)
        self.fragment_grads = bool(fragment_grads)

    def forward(self, verts, faces, verts_color, faces_opacity, mv_mats, proj_mats, verts_depth, faces_intense,
                tets, face_tets, tet_faces):
        f32, i32 = dict(dtype=th.float32), dict(dtype=th.int32)
        rows, shard = self._shard()
        out = _TetFn.apply(verts.to(**f32), faces.to(**i32), verts_color.to(**f32), faces_opacity.to(**f32),
                           mv_mats.to(**f32).transpose(1, 2), proj_mats.to(**f32).transpose(1, 2),
                           verts_depth.to(**f32), faces_intense.to(**f32),
                           tets.to(**i32), face_tets.to(**i32), tet_faces.to(**i32), self.render_settings,
                           rows, *_trailing(shard, self.full_grads, self.camera_grads, self.return_alpha, self.return_fragments,
                                            self.fragment_grads))
        return _outputs(out, self.return_alpha, self.return_fragments)

    _shard = TriRenderer._shard  # (rows, shard) of one device
