"""Shading from either renderer's per-pixel fragment lists (TriRenderer / TetRenderer(return_fragments=K), render_tri /
render_tet(..., return_fragments=K) -> Fragments(pix_to_face [B,K,H,W], bary [B,K,2,H,W], count [B,H,W])).

Plain torch and differentiable -- but for composite_fused, which is composite as one pair of HIP kernels (forward, backward:
csrc/dmr_shade.hip) without the [B,K,H,W,3,C] intermediates composite keeps for autograd, and composite_texture_fused, which
is composite_texture (a bilinear texture sampled at per-corner UVs, then blended) as another pair (csrc/dmr_texture.hip), and
face_visibility_fused, which is face_visibility (per-face sums of the blend weights, optionally weighted per pixel) and
face_coverage (per face the largest weight and the number of list slots that hold it) from one walk of the lists as a third
pair (csrc/dmr_visibility.hip): what a mesh optimiser reads to prune faces and to attribute per-pixel error to them.
interpolate_fused and composite_values_fused (csrc/dmr_interp.hip) are the two ENDS of a shader as kernels of their own, for a
deferred shader that fits none of the fused shapes: interpolate_fused is interpolate, the caller's own torch code then runs on
every fragment (an MLP, a lighting model), and composite_values_fused blends the per-slot results front to back
(composite_values is its torch model): composite_values(frag, o, interpolate(frag, faces, A), s) == composite(frag, faces, o, A, s).
A NEURAL shader (an MLP, a learned BRDF, a neural texture) wants rows [N,C], and only of the slots that hold a face: the packed
path (csrc/dmr_packed.hip).  pack_slots_fused numbers the used slots of the lists 0 .. n - 1 in the order of
pix_to_face.flatten(), interpolate_packed_fused writes one channel-last row per used slot, ready for nn.Linear, and
composite_values_packed_fused blends the rows the shader returns -- no permute, and nothing computed for an empty slot:
    packed = pack_slots_fused(frag, F)                                  # or capacity=M: no host wait, capturable
    x = interpolate_packed_fused(frag, packed, faces, features)         # [N,C]
    rgb = mlp(x)                                                        # [N,3], the caller's own torch code -- or
    rgb = mlp_rows_fused(x, weights, biases, n_rows=packed.n_used)      # a 1- or 2-hidden-layer MLP as one HIP kernel (RowMLP holds the parameters)
    image, T = composite_values_packed_fused(frag, packed, faces_opacity, rgb)
    color = image + T * bg.view(1, 3, 1, 1)
(pack_slots, interpolate_packed, composite_values_packed are the torch models, unpack_values the way back to [B,K,C,H,W]).
mlp_rows_fused (csrc/dmr_mlp.hip) is that MLP -- widths 16, 32 or 64, relu or tanh, an optional sigmoid on the output -- as one
forward and one backward kernel: the hidden activations stay in registers and the backward recomputes them, so nothing of size
[N,hidden] is written, read or kept for autograd; mlp_rows is its torch model, RowMLP the nn.Module that picks between them.
A LEARNED FIELD for that MLP to read -- this renderer's meshes change connectivity, so a UV atlas does not survive a step -- is a
multiresolution hash grid (Instant-NGP) sampled at every fragment's hit point, interpolate_packed_fused(frag, packed, faces, verts):
hashgrid_spec lays the table out (a HashGridSpec), hashgrid_rows is the torch model of the encoding [N,3] -> [N, L*F], hashgrid_rows_fused
(csrc/dmr_hashgrid.hip) the same as one forward and one backward kernel, HashGrid the nn.Module that owns the table:
    hit = interpolate_packed_fused(frag, packed, faces, verts)          # [N,3]; differentiable with fragment_grads=True
    rgb = mlp(grid(hit, n_rows=packed.n_used), n_rows=packed.n_used)    # grid = HashGrid(...), mlp = RowMLP(grid.out_features, 64, 3)
THE VIEW DIRECTION is that appearance model's other input -- without it the chain learns view-independent colour only: no
specular, no sheen.  A packed row does not know its view; packed_row_views_fused (packed_row_views is the torch model) tells, per
row, the view b of the slot that owns it.  sh_rows is the torch model of the encoding: per row w = x - origin[row_view], d = w / |w|,
and the degree^2 real spherical harmonics of d (tiny-cuda-nn's "SphericalHarmonics"); sh_rows_fused (csrc/dmr_sh.hip) the same as
one forward and one backward kernel, ViewSH the nn.Module, camera_origins the camera centres of the Modules' mv_mats (plain
torch through th.linalg.inv: dL/dorigin reaches mv_mats for pose refinement):
    view = FG.packed_row_views_fused(frag, packed)
    hit  = FG.interpolate_packed_fused(frag, packed, faces, verts)
    enc  = th.cat([grid(hit, n_rows=n), FG.ViewSH(4)(hit, FG.camera_origins(mv_mats), view, n_rows=n)], 1)
    image, T = FG.composite_values_packed_fused(frag, packed, faces_opacity, mlp(enc, n_rows=n))
THE BACKGROUND -- what shows between and through the faces wherever T > 0 -- is, without this, one constant RGB triple.  envmap_rows
is the torch model of a lookup from direction rows d [N,3] into a learnable lat-long (equirectangular) map [He,We,C], bilinear,
columns repeating and rows clamped, the pole axis z; envmap_rows_fused (csrc/dmr_envmap.hip) the same as one forward and one
backward kernel, EnvMap the nn.Module that owns the map, pixel_directions the world-space ray of every pixel centre in the
renderer's own convention (plain torch, differentiable to both matrices):
    env  = FG.EnvMap(256, 512).to(dev)                                   # render with settings.bg = 0
    dirs = FG.pixel_directions(mv_mats, proj_mats, H, W)                 # [B,H,W,3]
    bg   = env(dirs.reshape(-1, 3)).view(B, H, W, 3).permute(0, 3, 1, 2)
    color = image + T * bg                                               # image, T from any composite_* call (or 1 - alpha)
Fed a reflected or view direction per packed row (env(d, n_rows=n)) the same lookup is the cheapest specular term;
surface_packed_fused makes that direction.
THE SURFACE FRAME of every packed row -- the hit point, the unit geometric normal of its face turned towards the camera (these
meshes have no consistent winding) and the view ray mirrored at it -- is what an n.l term, a specular lookup, a Ref-NeRF-style
encoding or a normal loss start from.  surface_packed is the torch model, surface_packed_fused (csrc/dmr_surface.hip) the same as
one forward and one backward kernel, differentiable in verts, frag.bary and the camera centres; a slot's view is its b:
    s = FG.surface_packed_fused(frag, packed, faces, verts, FG.camera_origins(mv_mats))       # SurfaceRows(hit, normal, reflect), each [N,3]
    enc = th.cat([grid(s.hit, n_rows=n), FG.sh_rows_fused(s.reflect, 4, n_rows=n), s.normal], 1)
    rgb = mlp(enc, n_rows=n) + env(s.reflect, n_rows=n)                                       # diffuse + specular lookup
A ROUGH SURFACE needs that lookup in a blurred copy of the map, chosen per row: a single tap makes every surface a perfect mirror.
envmap_pyramid is the torch model of a mip pyramid [T,C] of the map (a 2 x 2 box chain in the map's own parameterisation, not a
GGX prefilter), envmap_lod_rows that of the trilinear lookup -- bilinear in two adjacent levels, linear in a level of detail per
row, differentiable in the direction, the level of detail and the pyramid; envmap_pyramid_fused and envmap_lod_rows_fused
(csrc/dmr_envmap_lod.hip) the same on HIP, EnvMapPyramid the nn.Module that owns the base map and builds the pyramid per call:
    s   = FG.surface_packed_fused(frag, packed, faces, verts, FG.camera_origins(mv_mats))
    out = mlp(enc, n_rows=n)                                  # [M,4]: rgb + roughness
    env = FG.EnvMapPyramid(256, 512).to(dev)
    spec = env(s.reflect, out[:, 3].sigmoid() * (env.levels - 1), n_rows=n)   # lod from roughness, the caller's mapping
    image, T = FG.composite_values_packed_fused(frag, packed, faces_opacity, out[:, :3] + spec)
What is HELD CONSTANT by every
function here -- it comes from the rasteriser as data, not as a function of the scene -- is
  * which faces a pixel blends (coverage, and where its walk stopped),
  * their order (the tile's depth sort),
  * the barycentrics (the (u, v) of the pixel's ray on each face: clamped to the face by the tri renderer, which blends every
    face its coverage test accepts; UNCLAMPED from the tet renderer, whose march crosses a face in its interior by
    construction) -- UNLESS the renderer was made with fragment_grads=True: frag.bary then requires grad, interpolate and
    composite (which only read it) pass the gradient on, and the renderer's backward carries it to verts and, with
    camera_grads, to mv_mats / proj_mats (tri: the exact derivative of the clamped (u, v), the clamp region held fixed; tet:
    that of the unclamped (u, v), and the option implies full_grads).  Positions, normals, texture coordinates or a depth
    shaded here then see the geometry,
exactly the constants of the renderer's own default gradients.  Gradients flow into what the caller passes: opacities,
per-vertex attributes, per-face scales.  A pixel with count > K holds the first K of its faces only: what is computed for it
is the truncated sum.

The tet renderer's lists are in exact march order, front to back; a pixel whose march failed (active == False) has count 0
and no fragments, and shades to the bare background like the renderer's own image.  interpolate(frag, faces, verts) is the
hit point of every fragment; with TetRenderer(fragment_grads=True) its gradient to verts is the hit point's full derivative
(the direct term through the vertex rows plus the movement of (u, v)), without it the direct term only.

The renderer's own colour, for pixels with count <= K:
    color, T = composite(frag, faces, faces_opacity, verts_color, face_scale=faces_intense);  color + T * bg.view(1, 3, 1, 1)
(and 1 - T its alpha).  The opacity-1 rule of the TET renderer is the one exception: behind a face of opacity 1 it goes on with
T = T_EPS / 10 = 1e-5 where the product here gives 0 -- the march ends at such a face, so it is the list's last, and the
renderer's colour and alpha differ from the lines above by 1e-5 bg and 1e-5 there.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional, Sequence, Tuple

import torch as th

__all__ = ["blend_weights", "interpolate", "composite", "face_visibility", "composite_fused", "composite_texture",
           "composite_texture_fused", "face_coverage", "face_visibility_fused", "composite_values", "interpolate_fused",
           "composite_values_fused", "PackedSlots", "pack_slots", "pack_slots_fused", "interpolate_packed", "interpolate_packed_fused",
           "composite_values_packed", "composite_values_packed_fused", "unpack_values", "mlp_rows", "mlp_rows_fused", "RowMLP",
           "HashGridSpec", "hashgrid_spec", "hashgrid_rows", "hashgrid_rows_fused", "HashGrid",
           "packed_row_views", "packed_row_views_fused", "sh_rows", "sh_rows_fused", "camera_origins", "ViewSH",
           "envmap_rows", "envmap_rows_fused", "EnvMap", "pixel_directions", "SurfaceRows", "surface_packed", "surface_packed_fused",
           "envmap_pyramid", "envmap_pyramid_fused", "envmap_lod_rows", "envmap_lod_rows_fused", "EnvMapPyramid"]

WRAPS = ("clamp", "repeat")  # the index into it is the C calls' `wrap`


def _opacity_slots(frag, faces_opacity: th.Tensor) -> Tuple[th.Tensor, th.Tensor]:
    """(used [B,K,H,W] bool, opacity of every slot's face with 0 in the empty ones)."""
    face = frag.pix_to_face
    used = face >= 0
    o = faces_opacity[face.clamp(min=0).long()]
    return used, th.where(used, o, th.zeros((), dtype=o.dtype, device=o.device))


def _transmittance(o: th.Tensor) -> th.Tensor:
    """[B,K+1,H,W]: prod_{j<k} (1 - o_j) for k = 0..K (the exclusive cumulative product over the slots, and the total)."""
    ones = th.ones_like(o[:, :1])
    return th.cat([ones, th.cumprod(1 - o, dim=1)], dim=1)


def blend_weights(frag, faces_opacity: th.Tensor) -> th.Tensor:
    """w_k = o_k * prod_{j<k} (1 - o_j) of every slot, [B,K,H,W]; 0 in empty slots.  frag: Fragments; faces_opacity [F].
    Constants: the faces and their order.  Differentiable in faces_opacity."""
    _, o = _opacity_slots(frag, faces_opacity)
    return o * _transmittance(o)[:, :-1]


def interpolate(frag, faces: th.Tensor, vert_attrs: th.Tensor) -> th.Tensor:
    """Per-vertex attributes vert_attrs [P,C] at every fragment, [B,K,C,H,W]: (1 - u - v) a_0 + u a_1 + v a_2 over the three
    vertices of the slot's face (faces [F,3]), with the renderer's (u, v) (tri: clamped; tet: as hit); 0 in empty slots.
    Constants: the faces and the barycentrics.  Differentiable in vert_attrs -- and in frag.bary when the renderer's
    fragment_grads made it differentiable."""
    face = frag.pix_to_face
    used = face >= 0
    vid = faces.long()[face.clamp(min=0).long()]             # [B,K,H,W,3]
    a = vert_attrs[vid]                                      # [B,K,H,W,3,C]
    u, v = frag.bary[:, :, 0].to(a.dtype), frag.bary[:, :, 1].to(a.dtype)
    w = th.stack([1 - u - v, u, v], dim=-1)                  # [B,K,H,W,3]
    out = (w.unsqueeze(-1) * a).sum(-2)                      # [B,K,H,W,C]
    out = out * used.unsqueeze(-1).to(a.dtype)
    return out.permute(0, 1, 4, 2, 3)


def composite(frag, faces: th.Tensor, faces_opacity: th.Tensor, vert_attrs: th.Tensor,
              face_scale: Optional[th.Tensor] = None) -> Tuple[th.Tensor, th.Tensor]:
    """Front-to-back blend of interpolated attributes: (sum_k w_k s_k a_k [B,C,H,W], T = prod_k (1 - o_k) [B,1,H,W]), a_k =
    interpolate(...), w_k = blend_weights(...), s_k = face_scale[b, face_k] (face_scale [B,F], e.g. faces_intense; None: 1).
    T is what is left for a background: result + T * bg (the tet renderer keeps 1e-5 behind a face of opacity 1, see the
    top).  Constants: the faces, their order, the barycentrics.
    Differentiable in faces_opacity, vert_attrs and face_scale (and in frag.bary with the renderer's fragment_grads)."""
    _, o = _opacity_slots(frag, faces_opacity)
    t = _transmittance(o)
    w = o * t[:, :-1]
    a = interpolate(frag, faces, vert_attrs)                 # [B,K,C,H,W]
    if face_scale is not None:
        idx = frag.pix_to_face.clamp(min=0).long()
        B = idx.shape[0]
        s = th.gather(face_scale, 1, idx.reshape(B, -1)).reshape(idx.shape)
        w = w * s.to(w.dtype)
    return (w.unsqueeze(2).to(a.dtype) * a).sum(1), t[:, -1:]


def composite_values(frag, faces_opacity: th.Tensor, values: th.Tensor, face_scale: Optional[th.Tensor] = None) -> Tuple[th.Tensor, th.Tensor]:
    """Front-to-back blend of per-slot values the caller computed, values [B,K,C,H,W] (the layout interpolate returns):
    (sum_k w_k s_k values_k [B,C,H,W], T = prod_k (1 - o_k) [B,1,H,W]) with w_k = blend_weights(...), s_k = face_scale[b, face_k]
    (face_scale [B,F]; None: 1) -- composite with the interpolation taken out:
        composite_values(frag, o, interpolate(frag, faces, A), s) == composite(frag, faces, o, A, s).
    The value of an empty slot is not read (masked, so a NaN there does not reach the image).  Any device, any float dtype.
    Constants: the faces and their order.  Differentiable in faces_opacity, values and face_scale."""
    used, o = _opacity_slots(frag, faces_opacity)
    t = _transmittance(o)
    w = o * t[:, :-1]
    if face_scale is not None:
        idx = frag.pix_to_face.clamp(min=0).long()
        B = idx.shape[0]
        w = w * th.gather(face_scale, 1, idx.reshape(B, -1)).reshape(idx.shape).to(w.dtype)
    v = th.where(used.unsqueeze(2), values, th.zeros((), dtype=values.dtype, device=values.device))
    return (w.unsqueeze(2).to(v.dtype) * v).sum(1), t[:, -1:]


def face_visibility(frag, faces_opacity: th.Tensor, F: int, pixel_weight: Optional[th.Tensor] = None) -> th.Tensor:
    """Sum of the blend weights every face received over a view's pixels, [B,F] (one scatter_add): 0 for a face no pixel
    blended (tet: no ray composited) -- the faces to prune.  Over all faces it sums to H * W - sum(T) per view.
    pixel_weight [B,H,W] multiplies every pixel's weights before the sum (a per-pixel error, say: its attribution to the faces);
    over all faces that sums to sum(pixel_weight * (1 - T)).  Constants: the faces and their order.
    Differentiable in faces_opacity and pixel_weight."""
    w = blend_weights(frag, faces_opacity)
    if pixel_weight is not None:
        w = w * pixel_weight.unsqueeze(1).to(w.dtype)
    B = w.shape[0]
    idx = frag.pix_to_face.clamp(min=0).long().reshape(B, -1)  # (empty slots add their weight 0 to face 0)
    return th.zeros(B, F, dtype=w.dtype, device=w.device).scatter_add(1, idx, w.reshape(B, -1))


def face_coverage(frag, faces_opacity: th.Tensor, F: int) -> Tuple[th.Tensor, th.Tensor]:
    """What pruning reads beside face_visibility, from the same lists: (max_weight [B,F], the largest blend weight any pixel
    gave the face, 0 for a face in no list; pixels [B,F] int64, the number of list slots that hold the face, whatever their
    weight).  Not differentiable.  Constants: the faces and their order."""
    w = blend_weights(frag, faces_opacity).detach()
    B = w.shape[0]
    used = (frag.pix_to_face >= 0).reshape(B, -1)
    idx = frag.pix_to_face.clamp(min=0).long().reshape(B, -1)
    w = th.where(used, w.reshape(B, -1), th.zeros((), dtype=w.dtype, device=w.device))
    max_weight = th.zeros(B, F, dtype=w.dtype, device=w.device).scatter_reduce(1, idx, w, "amax", include_self=True)
    pixels = th.zeros(B, F, dtype=th.int64, device=w.device).scatter_add(1, idx, used.long())
    return max_weight, pixels


class _CompositeFn(th.autograd.Function):
    """composite_fused's one Function over _C.composite_fragments / _C.composite_fragments_backward.  Arguments: pix_to_face, bary,
    faces, faces_opacity, vert_attrs, face_scale (a tensor or None)."""

    @staticmethod
    def forward(ctx, face, bary, faces, faces_opacity, vert_attrs, face_scale):
        image, t = _fused_kernels("composite").composite_fragments(face, bary, faces, faces_opacity, vert_attrs, face_scale)
        ctx.save_for_backward(face, bary, faces, faces_opacity, vert_attrs, *(() if face_scale is None else (face_scale,)))
        ctx.set_materialize_grads(False)  # an output the loss does not use arrives as None, and goes down as None: no zeros
        return image, t

    @staticmethod
    def backward(ctx, grad_image, grad_t):
        face, bary, faces, faces_opacity, vert_attrs, *scale = ctx.saved_tensors
        need = ctx.needs_input_grad  # (face, bary, faces, faces_opacity, vert_attrs, face_scale)
        need = (need[3], need[4], bool(scale) and need[5], need[1])
        if (grad_image is None and grad_t is None) or not any(need):
            return (None,) * 6
        d_op, d_attrs, d_scale, d_bary = _fused_kernels("composite").composite_fragments_backward(
            face, bary, faces, faces_opacity, vert_attrs, scale[0] if scale else None,
            None if grad_image is None else grad_image.contiguous(), None if grad_t is None else grad_t.contiguous(), need)
        return None, d_bary, None, d_op, d_attrs, d_scale


# torch path -> (the flag of `_C` that announces its fused pair of calls, what they fuse)
_FUSED = {"composite": ("SUPPORTS_FRAGMENT_COMPOSITE", "fragment"), "composite_texture": ("SUPPORTS_FRAGMENT_TEXTURE", "texture"),
          "face_visibility": ("SUPPORTS_FRAGMENT_VISIBILITY", "face-visibility"),
          "interpolate": ("SUPPORTS_FRAGMENT_DEFERRED", "fragment", "interpolation"),
          "composite_values": ("SUPPORTS_FRAGMENT_DEFERRED", "per-slot value"),
          "pack_slots": ("SUPPORTS_FRAGMENT_PACKED", "fragment", "slot packing"),
          "interpolate_packed": ("SUPPORTS_FRAGMENT_PACKED", "packed fragment", "interpolation"),
          "composite_values_packed": ("SUPPORTS_FRAGMENT_PACKED", "packed per-slot value"),
          "mlp_rows": ("SUPPORTS_FRAGMENT_MLP", "row", "MLP"),  # (a third entry: what stands for "compositing" in the message)
          "hashgrid_rows": ("SUPPORTS_FRAGMENT_HASHGRID", "row", "hash-grid encoding"),
          "packed_row_views": ("SUPPORTS_FRAGMENT_SH", "packed row", "view map"),
          "sh_rows": ("SUPPORTS_FRAGMENT_SH", "row", "spherical-harmonics encoding"),
          "envmap_rows": ("SUPPORTS_FRAGMENT_ENVMAP", "row", "environment-map lookup"),
          "envmap_pyramid": ("SUPPORTS_FRAGMENT_ENVMAP_LOD", "row", "environment-map pyramid"),
          "envmap_lod_rows": ("SUPPORTS_FRAGMENT_ENVMAP_LOD", "row", "environment-map lookup by level of detail"),
          "surface_packed": ("SUPPORTS_FRAGMENT_SURFACE", "packed row", "surface frame")}


def _fused_kernels(torch_path: str):
    """`_C` as the package holds it at call time (tests swap it), with the fused calls of `torch_path` -- or a TypeError."""
    from . import _impl
    c = _impl(None)
    flag, what, *noun = _FUSED[torch_path]
    if not getattr(c, flag, False):
        raise TypeError(f"{torch_path}_fused: the loaded libdmesh_renderer_hip.so / _C has no fused {what} {noun[0] if noun else 'compositing'}: rebuild "
                        f"(python -m dmesh_renderer_amd.build); fragments.{torch_path} is the torch path")
    return c


def _check_fused(name: str, torch_path: str, frag, faces, faces_opacity, face_scale, uv_faces, own_shapes, own_floats):
    """What both fused entry points refuse, in the order they refuse it: the lists' shapes, K, faces, uv_faces (None: not given),
    faces_opacity; the unit's own shapes (own_shapes() raises); face_scale's shape; float32 for the lists' floats, own_floats
    [(name, tensor)] and face_scale; int32 lists, integer faces / uv_faces; one HIP device for all.  -> (pix_to_face, bary)"""
    face, bary = frag.pix_to_face, frag.bary
    if face.dim() != 4:
        raise ValueError(f"{name}: frag.pix_to_face must be [B,K,H,W], got {tuple(face.shape)}")
    B, K, H, W = face.shape
    if tuple(bary.shape) != (B, K, 2, H, W):
        raise ValueError(f"{name}: frag.bary must be [B,K,2,H,W] = {(B, K, 2, H, W)}, got {tuple(bary.shape)}")
    if not 1 <= K <= 32:
        raise ValueError(f"{name}: K must be in 1..32, got {K}")
    if faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"{name}: faces must be [F,3], got {tuple(faces.shape)}")
    F = faces.shape[0]
    if uv_faces is not None and tuple(uv_faces.shape) != (F, 3):
        raise ValueError(f"{name}: uv_faces must be [F,3] = {(F, 3)}, got {tuple(uv_faces.shape)}")
    if tuple(faces_opacity.shape) != (F,):
        raise ValueError(f"{name}: faces_opacity must be [F] = {(F,)}, got {tuple(faces_opacity.shape)}")
    own_shapes()
    if face_scale is not None and tuple(face_scale.shape) != (B, F):
        raise ValueError(f"{name}: face_scale must be [B,F] = {(B, F)}, got {tuple(face_scale.shape)}")
    floats = [("frag.bary", bary), ("faces_opacity", faces_opacity)] + own_floats
    if face_scale is not None:
        floats.append(("face_scale", face_scale))
    for n, t in floats:
        if t.dtype != th.float32:
            raise TypeError(f"{name}: {n} must be float32, got {t.dtype}; {torch_path}")
    if face.dtype != th.int32:
        raise TypeError(f"{name}: frag.pix_to_face must be int32, got {face.dtype}; {torch_path}")
    ints = [("faces", faces)] + ([] if uv_faces is None else [("uv_faces", uv_faces)])
    for n, t in ints:
        if t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == th.bool:
            raise TypeError(f"{name}: {n} must be an integer tensor, got {t.dtype}; {torch_path}")
    for n, t in [("frag.pix_to_face", face)] + ints + floats:
        if not t.is_cuda or t.device != face.device:
            raise TypeError(f"{name}: {n} is on {t.device}: every tensor must be on one HIP device (there is no CPU path); {torch_path}")
    return face, bary


def composite_fused(frag, faces: th.Tensor, faces_opacity: th.Tensor, vert_attrs: th.Tensor,
                    face_scale: Optional[th.Tensor] = None) -> Tuple[th.Tensor, th.Tensor]:
    """composite(...) as one fused HIP kernel, and one for its backward: the same (sum_k w_k s_k a_k [B,C,H,W], T [B,1,H,W]),
    the same constants, gradients to faces_opacity, vert_attrs, face_scale and (with the renderer's fragment_grads) frag.bary --
    each computed only when autograd asks for it -- without composite's [B,K,H,W,3,C] intermediates.  K <= 32, 1 <= C <= 256
    (ValueError).  A slot whose face id lies outside [0, F) is empty, wherever it sits in the list; frag.count is not read.
    HIP float32 tensors only (pix_to_face int32; faces of another integer dtype are cast, as TriRenderer does): anything else
    is a TypeError -- composite is the torch path for it; nothing falls back silently."""
    _fused_kernels("composite")
    def own_shapes():
        if vert_attrs.dim() != 2:
            raise ValueError(f"composite_fused: vert_attrs must be [P,C], got {tuple(vert_attrs.shape)}")
        if not 1 <= vert_attrs.shape[1] <= 256:
            raise ValueError(f"composite_fused: C must be in 1..256, got {vert_attrs.shape[1]}")

    face, bary = _check_fused("composite_fused", "fragments.composite is the torch path for anything else", frag, faces, faces_opacity,
                              face_scale, None, own_shapes, [("vert_attrs", vert_attrs)])
    return _CompositeFn.apply(face, bary, faces.to(th.int32), faces_opacity, vert_attrs, face_scale)


def _wrap_index(i: th.Tensor, n: int, wrap: str) -> th.Tensor:
    return i.clamp(0, n - 1) if wrap == "clamp" else th.remainder(i, n)


def composite_texture(frag, faces: th.Tensor, faces_opacity: th.Tensor, vert_uvs: th.Tensor, texture: th.Tensor,
                      face_scale: Optional[th.Tensor] = None, *, uv_faces: Optional[th.Tensor] = None,
                      wrap: str = "clamp") -> Tuple[th.Tensor, th.Tensor]:
    """Front-to-back blend of a texture sampled at every fragment: (sum_k w_k s_k c_k [B,C,H,W], T [B,1,H,W]), with w_k, s_k,
    T and the empty-slot rule exactly those of composite, and c_k the bilinear sample of texture [Ht,Wt,C] (channel-last; one
    image shared by every view) at
        (s, t)_k = (1 - u - v) UV[c0] + u UV[c1] + v UV[c2],   (c0, c1, c2) = uv_faces[face_k],  UV = vert_uvs [Pu,2]
    uv_faces [F,3] holds per-corner rows of vert_uvs (the OBJ `vt` convention: seams work); None: faces.  Texel centres sit at
    half-integers, t = 0 is row 0 (no flip):
        x = s Wt - 0.5, x0 = floor(x), fx = x - x0, ix0 = wrap(x0, Wt), ix1 = wrap(x0 + 1, Wt)           (likewise y, t, Ht)
        c_k = (1-fy) ((1-fx) tex[iy0,ix0] + fx tex[iy0,ix1]) + fy ((1-fx) tex[iy1,ix0] + fx tex[iy1,ix1])
    wrap: "clamp" (indices clamped to [0, n-1]) or "repeat" (remainder mod n); fx, fy come from the unwrapped coordinate, so the
    derivative in x is the difference of the two wrapped texels -- 0 at a clamped border without a special case.
    Bilinear only: no mip levels, no nearest filter, no per-view textures.
    Constants: the faces, their order, the texel cell (the floor) -- and the barycentrics unless the renderer's fragment_grads
    made frag.bary differentiable.  Differentiable in faces_opacity, vert_uvs, texture, face_scale and frag.bary."""
    if wrap not in WRAPS:
        raise ValueError(f"composite_texture: wrap must be one of {WRAPS}, got {wrap!r}")
    face = frag.pix_to_face
    used = face >= 0
    _, o = _opacity_slots(frag, faces_opacity)
    t = _transmittance(o)
    w = o * t[:, :-1]
    idx = face.clamp(min=0).long()
    if face_scale is not None:
        B = idx.shape[0]
        w = w * th.gather(face_scale, 1, idx.reshape(B, -1)).reshape(idx.shape).to(w.dtype)
    Ht, Wt, _ = texture.shape
    uv = vert_uvs[(faces if uv_faces is None else uv_faces).long()[idx]]   # [B,K,H,W,3,2]
    u, v = frag.bary[:, :, 0].to(uv.dtype), frag.bary[:, :, 1].to(uv.dtype)
    st = (th.stack([1 - u - v, u, v], dim=-1).unsqueeze(-1) * uv).sum(-2)  # [B,K,H,W,2]
    x, y = st[..., 0] * Wt - 0.5, st[..., 1] * Ht - 0.5
    x0, y0 = th.floor(x.detach()), th.floor(y.detach())
    fx, fy = (x - x0).unsqueeze(-1), (y - y0).unsqueeze(-1)
    ix0, ix1 = _wrap_index(x0.long(), Wt, wrap), _wrap_index(x0.long() + 1, Wt, wrap)
    iy0, iy1 = _wrap_index(y0.long(), Ht, wrap), _wrap_index(y0.long() + 1, Ht, wrap)
    c = (1 - fy) * ((1 - fx) * texture[iy0, ix0] + fx * texture[iy0, ix1]) + fy * ((1 - fx) * texture[iy1, ix0] + fx * texture[iy1, ix1])
    c = c * used.unsqueeze(-1).to(c.dtype)                                  # [B,K,H,W,C]
    return (w.unsqueeze(-1).to(c.dtype) * c).sum(1).permute(0, 3, 1, 2), t[:, -1:]


class _CompositeTextureFn(th.autograd.Function):
    """composite_texture_fused's one Function over _C.composite_texture / _C.composite_texture_backward.  Arguments: pix_to_face,
    bary, uv_faces, faces_opacity, vert_uvs, texture, face_scale (a tensor or None), wrap (0 / 1)."""

    @staticmethod
    def forward(ctx, face, bary, uv_faces, faces_opacity, vert_uvs, texture, face_scale, wrap):
        image, t = _fused_kernels("composite_texture").composite_texture(face, bary, uv_faces, faces_opacity, vert_uvs, texture, face_scale, wrap)
        ctx.save_for_backward(face, bary, uv_faces, faces_opacity, vert_uvs, texture, *(() if face_scale is None else (face_scale,)))
        ctx.wrap = wrap
        ctx.set_materialize_grads(False)  # an output the loss does not use arrives as None, and goes down as None: no zeros
        return image, t

    @staticmethod
    def backward(ctx, grad_image, grad_t):
        face, bary, uv_faces, faces_opacity, vert_uvs, texture, *scale = ctx.saved_tensors
        need = ctx.needs_input_grad  # (face, bary, uv_faces, faces_opacity, vert_uvs, texture, face_scale, wrap)
        need = (need[3], need[4], need[5], bool(scale) and need[6], need[1])
        if (grad_image is None and grad_t is None) or not any(need):
            return (None,) * 8
        d_op, d_uvs, d_tex, d_scale, d_bary = _fused_kernels("composite_texture").composite_texture_backward(
            face, bary, uv_faces, faces_opacity, vert_uvs, texture, scale[0] if scale else None, ctx.wrap,
            None if grad_image is None else grad_image.contiguous(), None if grad_t is None else grad_t.contiguous(), need)
        return None, d_bary, None, d_op, d_uvs, d_tex, d_scale, None


def composite_texture_fused(frag, faces: th.Tensor, faces_opacity: th.Tensor, vert_uvs: th.Tensor, texture: th.Tensor,
                            face_scale: Optional[th.Tensor] = None, *, uv_faces: Optional[th.Tensor] = None,
                            wrap: str = "clamp") -> Tuple[th.Tensor, th.Tensor]:
    """composite_texture(...) as one fused HIP kernel, and one for its backward: the same (image [B,C,H,W], T [B,1,H,W]), the same
    constants, gradients to faces_opacity, vert_uvs, texture, face_scale and (with the renderer's fragment_grads) frag.bary --
    each computed only when autograd asks for it -- without the [B,K,H,W,C] samples and the index_put backward of the torch
    path.  Bilinear only: no mip levels, no nearest filter, no per-view textures.  K <= 32, 1 <= C <= 32, Ht, Wt >= 1,
    Ht * Wt * ceil(C / 4) < 2^32 - 1, wrap in {"clamp", "repeat"} (ValueError).  A slot whose face id lies outside [0, F) is
    empty, wherever it sits in the list; frag.count is not read.  Where a sample sits exactly on a texel-centre line the UV and
    barycentric gradients are those of the cell the float32 coordinate fell in.  HIP float32 tensors only (pix_to_face int32;
    faces / uv_faces of another integer dtype are cast): anything else is a TypeError -- composite_texture is the torch path
    for it; nothing falls back silently."""
    name = "composite_texture_fused"
    _fused_kernels("composite_texture")
    if wrap not in WRAPS:
        raise ValueError(f"{name}: wrap must be one of {WRAPS}, got {wrap!r}")

    def own_shapes():
        if vert_uvs.dim() != 2 or vert_uvs.shape[1] != 2:
            raise ValueError(f"{name}: vert_uvs must be [Pu,2], got {tuple(vert_uvs.shape)}")
        if texture.dim() != 3:
            raise ValueError(f"{name}: texture must be [Ht,Wt,C], got {tuple(texture.shape)}")
        Ht, Wt, C = texture.shape
        if not 1 <= C <= 32:
            raise ValueError(f"{name}: C must be in 1..32, got {C}")
        if Ht < 1 or Wt < 1 or Ht * Wt * ((C + 3) // 4) >= 2 ** 32 - 1:
            raise ValueError(f"{name}: texture must have Ht, Wt >= 1 and Ht * Wt * ceil(C / 4) < 2^32 - 1, got {tuple(texture.shape)}")

    face, bary = _check_fused(name, "fragments.composite_texture is the torch path for anything else", frag, faces, faces_opacity, face_scale,
                              uv_faces, own_shapes, [("vert_uvs", vert_uvs), ("texture", texture)])
    corners = faces if uv_faces is None else uv_faces
    return _CompositeTextureFn.apply(face, bary, corners.to(th.int32), faces_opacity, vert_uvs, texture, face_scale, WRAPS.index(wrap))


class _FaceVisibilityFn(th.autograd.Function):
    """face_visibility_fused's one Function over _C.face_visibility / _C.face_visibility_backward.  Arguments: pix_to_face,
    faces_opacity, pixel_weight (a tensor or None), coverage (bool) -> vis, or (vis, max_weight, pixels)."""

    @staticmethod
    def forward(ctx, face, faces_opacity, pixel_weight, coverage):
        vis, max_weight, pixels = _fused_kernels("face_visibility").face_visibility(face, faces_opacity, pixel_weight, coverage)
        ctx.save_for_backward(face, faces_opacity, *(() if pixel_weight is None else (pixel_weight,)))
        ctx.set_materialize_grads(False)  # an output the loss does not use arrives as None, and goes down as None: no zeros
        if not coverage:
            return vis
        ctx.mark_non_differentiable(max_weight, pixels)
        return vis, max_weight, pixels

    @staticmethod
    def backward(ctx, grad_vis, *_):
        face, faces_opacity, *weight = ctx.saved_tensors
        need = ctx.needs_input_grad  # (face, faces_opacity, pixel_weight, coverage)
        need = (need[1], bool(weight) and need[2])
        if grad_vis is None or not any(need):
            return (None,) * 4
        d_op, d_weight = _fused_kernels("face_visibility").face_visibility_backward(
            face, faces_opacity, weight[0] if weight else None, grad_vis.contiguous(), need)
        return None, d_op, d_weight, None


def face_visibility_fused(frag, faces_opacity: th.Tensor, F: int, pixel_weight: Optional[th.Tensor] = None, *, coverage: bool = False):
    """face_visibility(...) as one fused HIP kernel, and one for its backward, without the [B,K+1,H,W] transmittances and the
    scatter_add of B K H W weights: vis [B,F], differentiable in faces_opacity and pixel_weight [B,H,W] (None: 1), each gradient
    computed only when autograd asks for it.  coverage=True: (vis, max_weight [B,F], pixels [B,F] int32) -- face_coverage's two
    from the same walk, not differentiable.  A slot whose face id lies outside [0, F) is empty, wherever it sits in the list;
    frag.count and frag.bary are not read (bary may be None).  K <= 32, faces_opacity [F] (ValueError); F == 0 gives empty
    [B,0] tensors.  HIP float32 tensors only (pix_to_face int32): anything else is a TypeError -- face_visibility (and
    face_coverage) is the torch path for it; nothing falls back silently."""
    name = "face_visibility_fused"
    torch_path = "fragments.face_visibility (and face_coverage) is the torch path for anything else"
    _fused_kernels("face_visibility")
    face = frag.pix_to_face
    if face.dim() != 4:
        raise ValueError(f"{name}: frag.pix_to_face must be [B,K,H,W], got {tuple(face.shape)}")
    B, K, H, W = face.shape
    if not 1 <= K <= 32:
        raise ValueError(f"{name}: K must be in 1..32, got {K}")
    if isinstance(F, bool) or not isinstance(F, int) or F < 0:
        raise ValueError(f"{name}: F must be a non-negative int, got {F!r}")
    if tuple(faces_opacity.shape) != (F,):
        raise ValueError(f"{name}: faces_opacity must be [F] = {(F,)}, got {tuple(faces_opacity.shape)}")
    if pixel_weight is not None and tuple(pixel_weight.shape) != (B, H, W):
        raise ValueError(f"{name}: pixel_weight must be [B,H,W] = {(B, H, W)}, got {tuple(pixel_weight.shape)}")
    floats = [("faces_opacity", faces_opacity)] + ([] if pixel_weight is None else [("pixel_weight", pixel_weight)])
    for n, t in floats:
        if t.dtype != th.float32:
            raise TypeError(f"{name}: {n} must be float32, got {t.dtype}; {torch_path}")
    if face.dtype != th.int32:
        raise TypeError(f"{name}: frag.pix_to_face must be int32, got {face.dtype}; {torch_path}")
    for n, t in [("frag.pix_to_face", face)] + floats:
        if not t.is_cuda or t.device != face.device:
            raise TypeError(f"{name}: {n} is on {t.device}: every tensor must be on one HIP device (there is no CPU path); {torch_path}")
    if F == 0:  # nothing to launch
        vis = faces_opacity.new_zeros(B, 0)
        return (vis, faces_opacity.new_zeros(B, 0), th.zeros(B, 0, dtype=th.int32, device=face.device)) if coverage else vis
    return _FaceVisibilityFn.apply(face, faces_opacity, pixel_weight, bool(coverage))


class _InterpolateFn(th.autograd.Function):
    """The one Function of interpolate_fused (over _C.interpolate_fragments / _C.interpolate_fragments_backward) and of
    interpolate_packed_fused (over _C.interpolate_packed / _C.interpolate_packed_backward).  Arguments: pix_to_face, bary, faces,
    vert_attrs, and the packed call's row, n_used, rows -- three None for the dense one."""

    @staticmethod
    def forward(ctx, face, bary, faces, vert_attrs, row, n_used, rows):
        if row is None:
            out = _fused_kernels("interpolate").interpolate_fragments(face, bary, faces, vert_attrs)
        else:
            out = _fused_kernels("interpolate_packed").interpolate_packed(face, bary, row, n_used, faces, vert_attrs, rows)
        ctx.save_for_backward(face, bary, faces, vert_attrs, *(() if row is None else (row, n_used)))
        ctx.set_materialize_grads(False)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        face, bary, faces, vert_attrs, *packed = ctx.saved_tensors
        need = (ctx.needs_input_grad[3], ctx.needs_input_grad[1])  # (vert_attrs, bary)
        if grad_out is None or not any(need):
            return (None,) * 7
        if packed:
            d_attrs, d_bary = _fused_kernels("interpolate_packed").interpolate_packed_backward(face, bary, *packed, faces, vert_attrs,
                                                                                             grad_out.contiguous(), need)
        else:
            d_attrs, d_bary = _fused_kernels("interpolate").interpolate_fragments_backward(face, bary, faces, vert_attrs, grad_out.contiguous(), need)
        return None, d_bary, None, d_attrs, None, None, None


class _CompositeValuesFn(th.autograd.Function):
    """The one Function of composite_values_fused (over _C.composite_values / _C.composite_values_backward) and of
    composite_values_packed_fused (over _C.composite_values_packed / _C.composite_values_packed_backward).  Arguments: pix_to_face,
    faces_opacity, values, face_scale (a tensor or None), and the packed call's row, n_used -- two None for the dense one."""

    @staticmethod
    def forward(ctx, face, faces_opacity, values, face_scale, row, n_used):
        if row is None:
            image, t = _fused_kernels("composite_values").composite_values(face, faces_opacity, values, face_scale)
        else:
            image, t = _fused_kernels("composite_values_packed").composite_values_packed(face, row, faces_opacity, values, face_scale)
        ctx.packed = row is not None
        ctx.save_for_backward(face, faces_opacity, values, *((row, n_used) if ctx.packed else ()), *(() if face_scale is None else (face_scale,)))
        ctx.set_materialize_grads(False)  # an output the loss does not use arrives as None, and goes down as None: no zeros
        return image, t

    @staticmethod
    def backward(ctx, grad_image, grad_t):
        face, faces_opacity, values, *rest = ctx.saved_tensors
        packed, scale = (rest[:2], rest[2:]) if ctx.packed else ([], rest)
        need = ctx.needs_input_grad  # (face, faces_opacity, values, face_scale, row, n_used)
        need = (need[1], need[2], bool(scale) and need[3])
        if (grad_image is None and grad_t is None) or not any(need):
            return (None,) * 6
        tail = (faces_opacity, values, scale[0] if scale else None,
                None if grad_image is None else grad_image.contiguous(), None if grad_t is None else grad_t.contiguous(), need)
        if packed:
            d_op, d_values, d_scale = _fused_kernels("composite_values_packed").composite_values_packed_backward(face, *packed, *tail)
        else:
            d_op, d_values, d_scale = _fused_kernels("composite_values").composite_values_backward(face, *tail)
        return None, d_op, d_values, d_scale, None, None


def _check_lists(name: str, frag, bary_wanted: bool):
    """frag.pix_to_face [B,K,H,W] with K in 1..32 (and frag.bary [B,K,2,H,W]) -> B, K, H, W, or a ValueError."""
    face = frag.pix_to_face
    if face.dim() != 4:
        raise ValueError(f"{name}: frag.pix_to_face must be [B,K,H,W], got {tuple(face.shape)}")
    B, K, H, W = face.shape
    if bary_wanted and (frag.bary is None or tuple(frag.bary.shape) != (B, K, 2, H, W)):
        raise ValueError(f"{name}: frag.bary must be [B,K,2,H,W] = {(B, K, 2, H, W)}, got {None if frag.bary is None else tuple(frag.bary.shape)}")
    if not 1 <= K <= 32:
        raise ValueError(f"{name}: K must be in 1..32, got {K}")
    return B, K, H, W


def _check_tensors(name: str, torch_path: str, face, ints, floats):
    """float32 for `floats`, int32 lists, integer `ints` ([(name, tensor)]), one HIP device for all -- or a TypeError."""
    for n, t in floats:
        if t.dtype != th.float32:
            raise TypeError(f"{name}: {n} must be float32, got {t.dtype}; {torch_path}")
    if face.dtype != th.int32:
        raise TypeError(f"{name}: frag.pix_to_face must be int32, got {face.dtype}; {torch_path}")
    for n, t in ints:
        if t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == th.bool:
            raise TypeError(f"{name}: {n} must be an integer tensor, got {t.dtype}; {torch_path}")
    for n, t in [("frag.pix_to_face", face)] + ints + floats:
        if not t.is_cuda or t.device != face.device:
            raise TypeError(f"{name}: {n} is on {t.device}: every tensor must be on one HIP device (there is no CPU path); {torch_path}")


def _check_packed(name: str, torch_path: str, frag, packed) -> int:
    """packed.row of pix_to_face's shape, one n_used, rows an int >= 0 (ValueError); both int32 on the lists' device (TypeError)
    -> rows."""
    face = frag.pix_to_face
    if tuple(packed.row.shape) != tuple(face.shape):
        raise ValueError(f"{name}: packed.row must have frag.pix_to_face's shape {tuple(face.shape)}, got {tuple(packed.row.shape)}")
    if packed.n_used.numel() != 1:
        raise ValueError(f"{name}: packed.n_used must hold one element, got {tuple(packed.n_used.shape)}")
    if isinstance(packed.rows, bool) or not isinstance(packed.rows, int) or packed.rows < 0:
        raise ValueError(f"{name}: packed.rows must be a non-negative int, got {packed.rows!r}")
    for n, t in (("packed.row", packed.row), ("packed.n_used", packed.n_used)):
        if t.dtype != th.int32:
            raise TypeError(f"{name}: {n} must be int32, got {t.dtype}; {torch_path}")
    return packed.rows


def _check_interpolate(name: str, torch_path: str, frag, faces, vert_attrs, packed=None):
    """What interpolate_fused and (packed: a PackedSlots) interpolate_packed_fused refuse, in the order they refuse it
    -> packed.rows, or None."""
    _check_lists(name, frag, True)
    if faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"{name}: faces must be [F,3], got {tuple(faces.shape)}")
    if vert_attrs.dim() != 2:
        raise ValueError(f"{name}: vert_attrs must be [P,C], got {tuple(vert_attrs.shape)}")
    if not 1 <= vert_attrs.shape[1] <= 256:
        raise ValueError(f"{name}: C must be in 1..256, got {vert_attrs.shape[1]}")
    rows = None if packed is None else _check_packed(name, torch_path, frag, packed)
    ints = [("faces", faces)] + ([] if packed is None else [("packed.row", packed.row), ("packed.n_used", packed.n_used)])
    _check_tensors(name, torch_path, frag.pix_to_face, ints, [("frag.bary", frag.bary), ("vert_attrs", vert_attrs)])
    return rows


def _check_composite_values(name: str, torch_path: str, frag, faces_opacity, values, face_scale, packed=None):
    """What composite_values_fused (values [B,K,C,H,W]) and (packed: a PackedSlots) composite_values_packed_fused (values
    [packed.rows, C]) refuse, in the order they refuse it."""
    B, K, H, W = _check_lists(name, frag, False)
    if faces_opacity.dim() != 1:
        raise ValueError(f"{name}: faces_opacity must be [F], got {tuple(faces_opacity.shape)}")
    F = faces_opacity.shape[0]
    if packed is None:
        if values.dim() != 5 or tuple(values.shape[:2]) != (B, K) or tuple(values.shape[3:]) != (H, W):
            raise ValueError(f"{name}: values must be [B,K,C,H,W] = {(B, K, 'C', H, W)}, got {tuple(values.shape)}")
    else:
        rows = _check_packed(name, torch_path, frag, packed)
        if values.dim() != 2 or values.shape[0] != rows:
            raise ValueError(f"{name}: values must be [packed.rows, C] = {(rows, 'C')}, got {tuple(values.shape)}")
    C = values.shape[2 if packed is None else 1]
    if not 1 <= C <= 256:
        raise ValueError(f"{name}: C must be in 1..256, got {C}")
    if face_scale is not None and tuple(face_scale.shape) != (B, F):
        raise ValueError(f"{name}: face_scale must be [B,F] = {(B, F)}, got {tuple(face_scale.shape)}")
    floats = [("faces_opacity", faces_opacity), ("values", values)] + ([] if face_scale is None else [("face_scale", face_scale)])
    _check_tensors(name, torch_path, frag.pix_to_face, [] if packed is None else [("packed.row", packed.row), ("packed.n_used", packed.n_used)], floats)


def interpolate_fused(frag, faces: th.Tensor, vert_attrs: th.Tensor) -> th.Tensor:
    """interpolate(...) as one HIP kernel, and one for its backward: the same [B,K,C,H,W], 0 in empty slots, without the
    [B,K,H,W,3,C] gather interpolate keeps for autograd and without its index_put backward.  Gradients to vert_attrs and (with the
    renderer's fragment_grads) frag.bary, each computed only when autograd asks for it.  A slot whose face id lies outside [0, F)
    is empty, wherever it sits in the list, and a face whose row of `faces` holds a vertex index outside [0, P) gives 0;
    frag.count is not read.  K <= 32, 1 <= C <= 256 (ValueError).  HIP float32 tensors only (pix_to_face int32; faces of another
    integer dtype are cast): anything else is a TypeError -- interpolate is the torch path for it; nothing falls back silently."""
    name, torch_path = "interpolate_fused", "fragments.interpolate is the torch path for anything else"
    _fused_kernels("interpolate")
    _check_interpolate(name, torch_path, frag, faces, vert_attrs)
    return _InterpolateFn.apply(frag.pix_to_face, frag.bary, faces.to(th.int32), vert_attrs, None, None, None)


def composite_values_fused(frag, faces_opacity: th.Tensor, values: th.Tensor,
                           face_scale: Optional[th.Tensor] = None) -> Tuple[th.Tensor, th.Tensor]:
    """composite_values(...) as one HIP kernel, and one for its backward: the same (sum_k w_k s_k values_k [B,C,H,W], T [B,1,H,W]),
    the same constants, gradients to faces_opacity, values and face_scale -- each computed only when autograd asks for it --
    without the index_put backward of faces_opacity[face].  values is [B,K,C,H,W] (made contiguous if it is not).  A slot whose
    face id lies outside [0, F) is empty, wherever it sits in the list: its value is NOT READ (a NaN there reaches nothing) and
    its gradient is an exact 0.  A used slot of weight 0 (opacity 0, or behind a face of opacity 1) may skip its load: what a
    non-finite value there computes is unspecified.  frag.bary and frag.count are not read (bary may be None).  K <= 32,
    1 <= C <= 256 (ValueError).  HIP float32 tensors only (pix_to_face int32): anything else is a TypeError -- composite_values is
    the torch path for it; nothing falls back silently."""
    name, torch_path = "composite_values_fused", "fragments.composite_values is the torch path for anything else"
    _fused_kernels("composite_values")
    _check_composite_values(name, torch_path, frag, faces_opacity, values, face_scale)
    return _CompositeValuesFn.apply(frag.pix_to_face, faces_opacity, values, face_scale, None, None)


# ---------------------------------------------------------------------------
# Packed, channel-last rows: the used slots of the lists as rows 0 .. N - 1 of [N,C] tensors (csrc/dmr_packed.hip)
# ---------------------------------------------------------------------------
class PackedSlots(NamedTuple):
    """What pack_slots / pack_slots_fused return: which row of a packed [N,C] tensor every slot of the lists owns."""
    row: th.Tensor      # int32 [B,K,H,W]: the row of every used slot, -1 in an empty (or dropped) one
    n_used: th.Tensor   # int32 [1], on the lists' device: the number of used slots (may exceed `rows`: slots were dropped)
    rows: int           # N: the number of rows of every packed tensor made with this


def _capacity(name: str, capacity, face: th.Tensor):
    """capacity as given (None, or an int >= 0) -- None needs a host wait, which a stream capture cannot make."""
    if capacity is None:
        if face.is_cuda and th.cuda.is_current_stream_capturing():
            raise RuntimeError(f"{name}: capacity=None reads the number of used slots on the host, which a stream capture cannot do: "
                               f"pass capacity=M (the rows to provide for; n_used tells afterwards whether they sufficed)")
        return None
    if isinstance(capacity, bool) or not isinstance(capacity, int) or capacity < 0:
        raise ValueError(f"{name}: capacity must be None or a non-negative int, got {capacity!r}")
    return capacity


def _check_f(name: str, F):
    if isinstance(F, bool) or not isinstance(F, int) or F < 0:
        raise ValueError(f"{name}: F must be a non-negative int, got {F!r}")


def pack_slots(frag, F: int, capacity: Optional[int] = None) -> PackedSlots:
    """Numbers the used slots of the lists: a slot is USED when its face id lies in [0, F) (the empty-slot rule of every fused
    unit), and the used slots get the rows 0, 1, ... in the order of frag.pix_to_face.flatten(), that is (b, k, y, x).
    capacity=None: `rows` is the exact count (one host wait to read it; under stream capture a RuntimeError).  capacity=M: no
    host wait, rows = M, and a used slot whose row would be >= M gets row -1: it is DROPPED and behaves as empty in everything
    made with the result; n_used still holds the true count, so n_used > rows tells of the overflow.  Plain torch, any device."""
    face = frag.pix_to_face
    _check_f("pack_slots", F)
    capacity = _capacity("pack_slots", capacity, face)
    used = ((face >= 0) & (face < F)).reshape(-1)
    number = th.cumsum(used.to(th.int64), 0) - 1
    n_used = used.sum().to(th.int32).reshape(1)
    rows = int(n_used.item()) if capacity is None else capacity
    row = th.where(used & (number < rows), number, th.full_like(number, -1)).to(th.int32).reshape(face.shape)
    return PackedSlots(row, n_used, rows)


def _counting(frag, packed: PackedSlots, F: Optional[int]) -> th.Tensor:
    """[B,K,H,W] bool: the slots that count -- 0 <= row < rows, and (F given) a face id in [0, F)."""
    live = (packed.row >= 0) & (packed.row < packed.rows)
    if F is not None:
        live = live & (frag.pix_to_face >= 0) & (frag.pix_to_face < F)
    return live


def unpack_values(frag, packed: PackedSlots, values: th.Tensor) -> th.Tensor:
    """Packed rows values [N,C] back in the dense layout [B,K,C,H,W] interpolate returns: slot (b, k, y, x) holds
    values[packed.row[b, k, y, x]], 0 in a slot without a row.  Torch only (for tests and debugging); differentiable in values."""
    live = _counting(frag, packed, None)
    v = values[packed.row.clamp(min=0).long()]                  # [B,K,H,W,C]
    v = th.where(live.unsqueeze(-1), v, th.zeros((), dtype=v.dtype, device=v.device))
    return v.permute(0, 1, 4, 2, 3)


def interpolate_packed(frag, packed: PackedSlots, faces: th.Tensor, vert_attrs: th.Tensor) -> th.Tensor:
    """interpolate(...) on packed, channel-last rows, [N,C] with N = packed.rows: the row of a slot that counts (0 <= row < N and a
    face id in [0, F), F = len(faces)) holds its interpolated attributes, every other row is 0:
        interpolate_packed(frag, packed, faces, A) == interpolate(frag, faces, A).permute(0, 1, 3, 4, 2)[packed.row >= 0]
    for a `packed` made with capacity=None on the same lists and F (in general: those rows reordered by `row`, zeros in the rest).
    Constants and gradients as interpolate's.  Plain torch, any device, any float dtype."""
    live = _counting(frag, packed, faces.shape[0])
    face = th.where(live, frag.pix_to_face, th.full_like(frag.pix_to_face, -1))
    dense = interpolate(frag._replace(pix_to_face=face), faces, vert_attrs).permute(0, 1, 3, 4, 2)   # [B,K,H,W,C]
    out = dense.new_zeros(packed.rows, vert_attrs.shape[1])
    return out.index_put((packed.row[live].long(),), dense[live])


def composite_values_packed(frag, packed: PackedSlots, faces_opacity: th.Tensor, values: th.Tensor,
                            face_scale: Optional[th.Tensor] = None) -> Tuple[th.Tensor, th.Tensor]:
    """composite_values(...) over packed rows values [N,C] (N = packed.rows): (image [B,C,H,W], T [B,1,H,W]) with
        composite_values_packed(frag, packed, o, v, s) == composite_values(frag', o, unpack_values(frag, packed, v), s)
    where frag' is frag with every slot that does not count (no row in [0, N), or a face id outside [0, F), F = len(faces_opacity))
    set to -1: a dropped slot is skipped by the blend, as an empty one.  Differentiable in faces_opacity, values and face_scale."""
    live = _counting(frag, packed, faces_opacity.shape[0])
    face = th.where(live, frag.pix_to_face, th.full_like(frag.pix_to_face, -1))
    return composite_values(frag._replace(pix_to_face=face), faces_opacity, unpack_values(frag, packed, values), face_scale)


def pack_slots_fused(frag, F: int, capacity: Optional[int] = None) -> PackedSlots:
    """pack_slots(...) as three stream-ordered HIP launches (per-workgroup counts, one workgroup's scan, the rows): the same
    row, n_used and rows, exactly.  capacity=None waits for the device once, to read the count (under stream capture a
    RuntimeError: pass capacity=M); capacity=M never waits.  K <= 32, B K H W < 2^31 (ValueError).  HIP int32 lists only: anything else
    is a TypeError -- pack_slots is the torch path for it; nothing falls back silently.  frag.bary and frag.count are not read."""
    name, torch_path = "pack_slots_fused", "fragments.pack_slots is the torch path for anything else"
    c = _fused_kernels("pack_slots")
    B, K, H, W = _check_lists(name, frag, False)
    _check_f(name, F)
    if B * K * H * W >= 2 ** 31 or F >= 2 ** 31:
        raise ValueError(f"{name}: B K H W and F must be below 2^31, got {B * K * H * W} slots, F = {F}")
    face = frag.pix_to_face
    _check_tensors(name, torch_path, face, [], [])
    capacity = _capacity(name, capacity, face)
    if B * H * W == 0:
        return PackedSlots(th.full_like(face, -1), th.zeros(1, dtype=th.int32, device=face.device), capacity or 0)
    row, n_used = c.pack_slots(face, F, B * K * H * W if capacity is None else capacity)
    return PackedSlots(row, n_used, int(n_used.item()) if capacity is None else capacity)


def interpolate_packed_fused(frag, packed: PackedSlots, faces: th.Tensor, vert_attrs: th.Tensor) -> th.Tensor:
    """interpolate_packed(...) as one HIP kernel, and one for its backward: the same [N,C] channel-last rows, what nn.Linear
    takes, without the [B,K,C,H,W] tensor and its permute.  A slot counts only if 0 <= row < N and its face id lies in [0, F): a
    `packed` made for another F or capacity stays in bounds; a slot with a row that does not count, and a face whose row of
    `faces` holds a vertex index outside [0, P), gives a row of zeros.  Rows [min(n_used, N), N) are exact zeros (the count is
    read on the device).  Gradients to vert_attrs and (with the renderer's fragment_grads) frag.bary, each computed only when
    autograd asks for it; dL_dbary is an exact 0 in empty and dropped slots.  N == 0 gives an empty [0,C] tensor without a launch
    (it carries no gradient).  K <= 32, 1 <= C <= 256, packed.row of pix_to_face's shape (ValueError).  HIP float32 / int32 tensors
    on one device only: anything else is a TypeError -- interpolate_packed is the torch path for it; nothing falls back silently."""
    name, torch_path = "interpolate_packed_fused", "fragments.interpolate_packed is the torch path for anything else"
    _fused_kernels("interpolate_packed")
    rows = _check_interpolate(name, torch_path, frag, faces, vert_attrs, packed)
    if rows == 0:
        return vert_attrs.new_zeros((0, vert_attrs.shape[1]))
    return _InterpolateFn.apply(frag.pix_to_face, frag.bary, faces.to(th.int32), vert_attrs, packed.row, packed.n_used, rows)


def composite_values_packed_fused(frag, packed: PackedSlots, faces_opacity: th.Tensor, values: th.Tensor,
                                  face_scale: Optional[th.Tensor] = None) -> Tuple[th.Tensor, th.Tensor]:
    """composite_values_packed(...) as one HIP kernel, and one for its backward: the same (image [B,C,H,W], T [B,1,H,W]) from
    packed rows values [N,C] (made contiguous if they are not), N = packed.rows.  A slot counts only if 0 <= row < N and its face
    id lies in [0, F); every other slot is skipped, its row (if it has one) is NOT READ and gets exact zeros in dL_dvalues, as do
    the rows [min(n_used, N), N).  A counting slot of weight 0 (opacity 0, or behind a face of opacity 1) may skip its load.
    Gradients to faces_opacity, values and face_scale, each computed only when autograd asks for it.  frag.bary and frag.count are
    not read.  K <= 32, 1 <= C <= 256, values [packed.rows, C] (ValueError).  HIP float32 / int32 tensors on one device only:
    anything else is a TypeError -- composite_values_packed is the torch path for it; nothing falls back silently."""
    name, torch_path = "composite_values_packed_fused", "fragments.composite_values_packed is the torch path for anything else"
    _fused_kernels("composite_values_packed")
    _check_composite_values(name, torch_path, frag, faces_opacity, values, face_scale, packed)
    return _CompositeValuesFn.apply(frag.pix_to_face, faces_opacity, values, face_scale, packed.row, packed.n_used)


# ---------------------------------------------------------------------------
# A small MLP over packed rows: the shader between interpolate_packed_fused and composite_values_packed_fused (csrc/dmr_mlp.hip)
# ---------------------------------------------------------------------------
ACTIVATIONS = ("relu", "tanh")        # the index into it is the C calls' `act`
OUT_ACTIVATIONS = ("none", "sigmoid")  # ... and `oact`
MLP_HIDDEN = (16, 32, 64)             # the fused kernels' hidden widths; 1 <= Cin <= 64, 1 <= Cout <= 16


def _check_n_rows(name: str, n_rows):
    """The last of what the torch and the fused path of every row function (mlp_rows, hashgrid_rows, sh_rows, envmap_rows) both refuse."""
    if n_rows is not None and (not isinstance(n_rows, th.Tensor) or n_rows.numel() != 1):
        raise ValueError(f"{name}: n_rows must be None or a tensor of one element, got {tuple(n_rows.shape) if isinstance(n_rows, th.Tensor) else n_rows!r}")


def _check_row_tensors(name: str, torch_path: str, x, floats, ints):
    """What the fused row functions refuse after their arguments' shapes, in this order: N (ValueError), then (TypeError) the
    float32 tensors `floats`, the int32 tensors `ints`, one HIP device for all; both are lists of (name, tensor or None), x first."""
    floats, ints = ([(n, t) for n, t in tensors if t is not None] for tensors in (floats, ints))
    if x.shape[0] >= 2 ** 31:
        raise ValueError(f"{name}: N must be below 2^31, got {x.shape[0]}; {torch_path}")
    for tensors, dtype, word in ((floats, th.float32, "float32"), (ints, th.int32, "int32")):
        for n, t in tensors:
            if t.dtype != dtype:
                raise TypeError(f"{name}: {n} must be {word}, got {t.dtype}; {torch_path}")
    for n, t in floats + ints:
        if not t.is_cuda or t.device != x.device:
            raise TypeError(f"{name}: {n} is on {t.device}: every tensor must be on one HIP device (there is no CPU path); {torch_path}")


def _save_optional(ctx, *tensors):
    """save_for_backward for tensors of which some are None ..."""
    ctx.saved_mask = tuple(t is not None for t in tensors)
    ctx.save_for_backward(*(t for t in tensors if t is not None))


def _saved_optional(ctx):
    """... and the same tuple back, None where it was."""
    saved = iter(ctx.saved_tensors)
    return tuple(next(saved) if has else None for has in ctx.saved_mask)


def _mlp_arguments(name: str, x, weights, biases, activation, out_activation, n_rows):
    """What mlp_rows and mlp_rows_fused both refuse (ValueError), in this order: the number of weights and biases, the
    activations' names, x [N,Cin], the weights' chain of shapes [out_l, in_l] with one hidden width, the biases' shapes, n_rows.
    -> (weights, biases) as tuples."""
    weights, biases = tuple(weights), tuple(biases)
    if len(weights) not in (2, 3):
        raise ValueError(f"{name}: weights must hold 2 or 3 tensors (1 or 2 hidden layers), got {len(weights)}")
    if len(biases) != len(weights):
        raise ValueError(f"{name}: biases must hold one entry (a tensor or None) per weight, got {len(biases)} for {len(weights)}")
    if activation not in ACTIVATIONS:
        raise ValueError(f"{name}: activation must be one of {ACTIVATIONS}, got {activation!r}")
    if out_activation not in OUT_ACTIVATIONS:
        raise ValueError(f"{name}: out_activation must be one of {OUT_ACTIVATIONS}, got {out_activation!r}")
    if x.dim() != 2:
        raise ValueError(f"{name}: x must be [N,Cin], got {tuple(x.shape)}")
    if any(w.dim() != 2 for w in weights):
        raise ValueError(f"{name}: every weight must be [out,in], got {[tuple(w.shape) for w in weights]}")
    hidden, c_out, c_in = weights[0].shape[0], weights[-1].shape[0], x.shape[1]
    for l, (w, b) in enumerate(zip(weights, biases)):
        want = (c_out if l == len(weights) - 1 else hidden, c_in if l == 0 else hidden)
        if tuple(w.shape) != want:
            raise ValueError(f"{name}: weights[{l}] must be [out,in] = {want} (x is {tuple(x.shape)}, one hidden width), got {tuple(w.shape)}")
        if b is not None and tuple(b.shape) != want[:1]:
            raise ValueError(f"{name}: biases[{l}] must be [out] = {want[:1]} or None, got {tuple(b.shape)}")
    _check_n_rows(name, n_rows)
    return weights, biases


def mlp_rows(x: th.Tensor, weights: Sequence[th.Tensor], biases: Sequence[Optional[th.Tensor]], *, activation: str = "relu",
             out_activation: str = "none", n_rows: Optional[th.Tensor] = None) -> th.Tensor:
    """A small MLP over rows x [N,Cin] -> [N,Cout]: y = oact(W_L act(... act(W_1 x + b_1)) + b_L), weights W_l [out_l, in_l] in
    nn.Linear's layout (2 or 3 of them: 1 or 2 hidden layers of one width), biases [out_l] or None each; activation "relu" or
    "tanh", out_activation "none" or "sigmoid".  n_rows (None, or an integer tensor of one element on x's device -- what
    PackedSlots.n_used is): the rows r >= min(max(n_rows, 0), N) are NOT READ -- a NaN there reaches nothing --, give exact zeros
    in y and in dL_dx and add nothing to the gradient of any weight or bias; y[:n] is the MLP of x[:n].  With capacity=M the tail
    rows of interpolate_packed's result are zeros, which a bias turns into non-zero outputs: without n_rows they would enter
    dL_db and dL_dW.  The count is used on the device (no host wait).  Plain torch, any device, any float dtype: the model
    mlp_rows_fused is tested against."""
    weights, biases = _mlp_arguments("mlp_rows", x, weights, biases, activation, out_activation, n_rows)
    mask = None
    h = x
    if n_rows is not None:
        mask = (th.arange(x.shape[0], device=x.device) < n_rows.reshape(1).clamp(min=0)).unsqueeze(1)
        h = th.where(mask, x, th.zeros((), dtype=x.dtype, device=x.device))
    for l, (w, b) in enumerate(zip(weights, biases)):
        h = h @ w.t()
        if b is not None:
            h = h + b
        if l < len(weights) - 1:
            h = th.relu(h) if activation == "relu" else th.tanh(h)
    if out_activation == "sigmoid":
        h = th.sigmoid(h)
    return h if mask is None else th.where(mask, h, th.zeros((), dtype=h.dtype, device=h.device))


class _MlpRowsFn(th.autograd.Function):
    """mlp_rows_fused over _C.mlp_rows / _C.mlp_rows_backward.  Arguments: x, n_rows (a tensor or None), act, oact, the number of
    weights L, then the L weights and the L biases (a tensor or None each).  Nothing but the inputs is saved."""

    @staticmethod
    def forward(ctx, x, n_rows, act, oact, L, *params):
        weights, biases = params[:L], params[L:]
        y = _fused_kernels("mlp_rows").mlp_rows(x, list(weights), list(biases), act, oact, n_rows)
        ctx.meta = (act, oact, L)
        _save_optional(ctx, x, *weights, *biases, n_rows)
        ctx.set_materialize_grads(False)  # an output the loss does not use arrives as None, and goes down as None: no launch
        return y

    @staticmethod
    def backward(ctx, grad_y):
        act, oact, L = ctx.meta
        need = ctx.needs_input_grad
        need_x, need_w = need[0], list(need[5:5 + L])
        need_b = [ctx.saved_mask[1 + L + l] and need[5 + L + l] for l in range(L)]
        if grad_y is None or not (need_x or any(need_w) or any(need_b)):
            return (None,) * (5 + 2 * L)
        x, *params, n_rows = _saved_optional(ctx)
        weights, biases = params[:L], params[L:]
        dx, gw, gb = _fused_kernels("mlp_rows").mlp_rows_backward(x, weights, biases, act, oact, n_rows, grad_y.contiguous(), need_x, need_w, need_b)
        return (dx, None, None, None, None, *gw, *gb)


def mlp_rows_fused(x: th.Tensor, weights: Sequence[th.Tensor], biases: Sequence[Optional[th.Tensor]], *, activation: str = "relu",
                   out_activation: str = "none", n_rows: Optional[th.Tensor] = None) -> th.Tensor:
    """mlp_rows(...) as one HIP kernel, and one for its backward (plus a small one that sums the workgroups' weight-gradient
    sums in f64): a lane owns a row, the hidden activations live in its registers and never reach memory, and the backward
    recomputes them from x -- autograd keeps x, the weights and nothing of size [N,hidden].  The same y, the same n_rows rule
    (read on the device: no host wait, capturable; a negative count is 0), gradients to x, every weight and every bias, each
    computed only when autograd asks for it.  Hidden width 16, 32 or 64, 1 <= Cin <= 64, 1 <= Cout <= 16, N >= 0 (ValueError).  HIP
    float32 tensors on one device only (n_rows int32 [1]), made contiguous if they are not: anything else is a TypeError --
    mlp_rows is the torch path for it; nothing falls back silently."""
    name, torch_path = "mlp_rows_fused", "fragments.mlp_rows is the torch path for anything else"
    _fused_kernels("mlp_rows")
    weights, biases = _mlp_arguments(name, x, weights, biases, activation, out_activation, n_rows)
    hidden, c_in, c_out = weights[0].shape[0], x.shape[1], weights[-1].shape[0]
    if hidden not in MLP_HIDDEN:
        raise ValueError(f"{name}: the hidden width must be one of {MLP_HIDDEN}, got {hidden}; {torch_path}")
    if not 1 <= c_in <= 64:
        raise ValueError(f"{name}: Cin must be in 1..64, got {c_in}; {torch_path}")
    if not 1 <= c_out <= 16:
        raise ValueError(f"{name}: Cout must be in 1..16, got {c_out}; {torch_path}")
    floats = [("x", x)] + [(f"weights[{l}]", w) for l, w in enumerate(weights)] + [(f"biases[{l}]", b) for l, b in enumerate(biases)]
    _check_row_tensors(name, torch_path, x, floats, [("n_rows", n_rows)])
    return _MlpRowsFn.apply(x, None if n_rows is None else n_rows.reshape(1), ACTIVATIONS.index(activation), OUT_ACTIVATIONS.index(out_activation),
                            len(weights), *weights, *biases)


class RowMLP(th.nn.Module):
    """The parameters of mlp_rows / mlp_rows_fused as a Module, so that an optimizer can own them: c_in -> hidden (x n_hidden, 1 or
    2) -> c_out, nn.Linear's layout and initialisation.  forward(x, n_rows=None) runs mlp_rows_fused on HIP float32 rows and
    mlp_rows on anything else.  from_sequential(seq) takes over the Linear layers of an nn.Sequential (it shares their
    Parameters); to_sequential() is the way back."""

    def __init__(self, c_in: int, hidden: int, c_out: int, n_hidden: int = 1, activation: str = "relu", out_activation: str = "none",
                 bias: bool = True):
        super().__init__()
        if n_hidden not in (1, 2):
            raise ValueError(f"RowMLP: n_hidden must be 1 or 2, got {n_hidden!r}")
        if activation not in ACTIVATIONS or out_activation not in OUT_ACTIVATIONS:
            raise ValueError(f"RowMLP: activation must be one of {ACTIVATIONS} and out_activation one of {OUT_ACTIVATIONS}, "
                             f"got {activation!r}, {out_activation!r}")
        self.activation, self.out_activation = activation, out_activation
        dims = [c_in] + [hidden] * n_hidden + [c_out]
        layers = [th.nn.Linear(i, o, bias=bias) for i, o in zip(dims[:-1], dims[1:])]  # (for their initialisation)
        self.weights = th.nn.ParameterList([l.weight for l in layers])
        self.biases = th.nn.ParameterList([l.bias for l in layers]) if bias else None

    def _biases(self):
        return [None] * len(self.weights) if self.biases is None else list(self.biases)

    def forward(self, x: th.Tensor, n_rows: Optional[th.Tensor] = None) -> th.Tensor:
        f = mlp_rows_fused if (x.is_cuda and x.dtype == th.float32) else mlp_rows
        return f(x, list(self.weights), self._biases(), activation=self.activation, out_activation=self.out_activation, n_rows=n_rows)

    @classmethod
    def from_sequential(cls, seq: th.nn.Sequential) -> "RowMLP":
        """An nn.Sequential of Linear, ReLU / Tanh, [Linear, ReLU / Tanh,] Linear [, Sigmoid] -> a RowMLP on the same Parameters."""
        mods = list(seq)
        out_activation = "none"
        if mods and isinstance(mods[-1], th.nn.Sigmoid):
            out_activation, mods = "sigmoid", mods[:-1]
        linears, acts = mods[0::2], mods[1::2]
        names = {th.nn.ReLU: "relu", th.nn.Tanh: "tanh"}
        if (len(mods) not in (3, 5) or not all(isinstance(m, th.nn.Linear) for m in linears) or not all(type(m) in names for m in acts)
                or len({type(m) for m in acts}) != 1):
            raise ValueError("RowMLP.from_sequential: expected Linear, ReLU|Tanh, [Linear, the same activation,] Linear [, Sigmoid], got "
                             + ", ".join(type(m).__name__ for m in seq))
        has = {l.bias is not None for l in linears}
        if len(has) != 1 or len({l.out_features for l in linears[:-1]}) != 1:
            raise ValueError("RowMLP.from_sequential: the Linear layers must all have a bias or all have none, and one hidden width")
        m = cls(linears[0].in_features, linears[0].out_features, linears[-1].out_features, n_hidden=len(linears) - 1,
                activation=names[type(acts[0])], out_activation=out_activation, bias=has.pop())
        m.weights = th.nn.ParameterList([l.weight for l in linears])
        if m.biases is not None:
            m.biases = th.nn.ParameterList([l.bias for l in linears])
        return m

    def to_sequential(self) -> th.nn.Sequential:
        """The same network as an nn.Sequential of Linear layers on the same Parameters."""
        mods = []
        for l, (w, b) in enumerate(zip(self.weights, self._biases())):
            lin = th.nn.Linear(w.shape[1], w.shape[0], bias=b is not None, device="meta")
            lin.weight = w
            if b is not None:
                lin.bias = b
            mods.append(lin)
            if l < len(self.weights) - 1:
                mods.append(th.nn.ReLU() if self.activation == "relu" else th.nn.Tanh())
        if self.out_activation == "sigmoid":
            mods.append(th.nn.Sigmoid())
        return th.nn.Sequential(*mods)


# ---------------------------------------------------------------------------
# A multiresolution hash grid over packed rows of 3-D points: the learned field in front of the MLP (csrc/dmr_hashgrid.hip)
# ---------------------------------------------------------------------------
HASH_PRIMES = (1, 2654435761, 805459861)  # per axis; the products are taken modulo 2^32
HASHGRID_FEATURES = (1, 2, 4, 8)          # F; 1 <= L <= 16, L * F <= 64 (RowMLP's Cin), 4 <= log2_T <= 24, 1 <= R_l <= 65536


class HashGridSpec(NamedTuple):
    """The layout of a hash grid's table (hashgrid_spec): per level its resolution and its number of rows, the running sums of
    those (offsets[L] = the rows of the table), the features per row and log2 of the hashed levels' size."""
    resolutions: Tuple[int, ...]
    sizes: Tuple[int, ...]
    offsets: Tuple[int, ...]
    features: int
    log2_table_size: int


def hashgrid_spec(n_levels: int = 16, features: int = 2, log2_table_size: int = 19, base_resolution: int = 16,
                  per_level_scale: float = 1.38) -> HashGridSpec:
    """The layout of a multiresolution hash grid (Instant-NGP) of n_levels = L levels with F = features floats per grid vertex:
    level l has resolution R_l = floor(base_resolution * per_level_scale**l) (float64) -- R_l cells and R_l + 1 vertices per axis
    over the unit cube -- and, with T = 2**log2_table_size, is DENSE when (R_l + 1)^3 <= T: (R_l + 1)^3 rows, vertex (ix, iy, iz)
    in row ix + (R_l + 1) (iy + (R_l + 1) iz); else HASHED: T rows, the vertex in row ((ix * 1) ^ (iy * 2654435761) ^
    (iz * 805459861)) & (T - 1), the products modulo 2^32.  The table is one tensor [offsets[L], F], level l owns the rows
    [offsets[l], offsets[l+1]).  ValueError, in this order, unless 1 <= L <= 16, F in {1, 2, 4, 8}, L * F <= 64,
    4 <= log2_table_size <= 24 and 1 <= R_l <= 65536.  Computed on the host; the C library states the same rule
    (dmr_hashgrid_layout) and a test holds the two equal."""
    name = "hashgrid_spec"
    L, F, log2_T = int(n_levels), int(features), int(log2_table_size)
    if not 1 <= L <= 16:
        raise ValueError(f"{name}: n_levels must be in 1..16, got {n_levels!r}")
    if F not in HASHGRID_FEATURES:
        raise ValueError(f"{name}: features must be one of {HASHGRID_FEATURES}, got {features!r}")
    if L * F > 64:
        raise ValueError(f"{name}: n_levels * features must be at most 64 (RowMLP's Cin), got {L * F}")
    if not 4 <= log2_T <= 24:
        raise ValueError(f"{name}: log2_table_size must be in 4..24, got {log2_table_size!r}")
    resolutions = tuple(int(math.floor(float(base_resolution) * float(per_level_scale) ** l)) for l in range(L))
    for l, r in enumerate(resolutions):
        if not 1 <= r <= 65536:
            raise ValueError(f"{name}: the resolution of level {l} must be in 1..65536, got {r}")
    T = 1 << log2_T
    sizes = tuple((r + 1) ** 3 if (r + 1) ** 3 <= T else T for r in resolutions)
    offsets = [0]
    for s in sizes:
        offsets.append(offsets[-1] + s)
    return HashGridSpec(resolutions, sizes, tuple(offsets), F, log2_T)


def _hashgrid_arguments(name: str, x, table, spec, n_rows):
    """What hashgrid_rows and hashgrid_rows_fused both refuse (ValueError), in this order: the spec's type, x [N,3], table
    [offsets[L], F], n_rows."""
    if not isinstance(spec, HashGridSpec):
        raise ValueError(f"{name}: spec must be a HashGridSpec (hashgrid_spec(...)), got {type(spec).__name__}")
    if x.dim() != 2 or x.shape[1] != 3:
        raise ValueError(f"{name}: x must be [N,3], got {tuple(x.shape)}")
    want = (spec.offsets[-1], spec.features)
    if tuple(table.shape) != want:
        raise ValueError(f"{name}: table must be [offsets[L], F] = {want}, got {tuple(table.shape)}")
    _check_n_rows(name, n_rows)


def hashgrid_rows(x: th.Tensor, table: th.Tensor, spec: HashGridSpec, n_rows: Optional[th.Tensor] = None) -> th.Tensor:
    """The multiresolution hash-grid encoding of rows x [N,3] of points of the unit cube -> [N, L*F], level-major channels: per
    level l and coordinate u, u_c = clamp(u, 0, 1) with NaN counting as 0, p = u_c R_l, i = min(floor(p), R_l - 1), t = p - i in
    [0, 1] (a point on the upper face lands in the last cell with t = 1), and
        y[r, l F + f] = sum over the 8 corners c of w_c table[offsets[l] + row_l(i + c), f]
    with the trilinear w_c = (wx wy) wz from (t_x, t_y, t_z) and row_l of hashgrid_spec (index arithmetic in int64 with explicit
    & 0xffffffff).  Differentiable in table (a scatter of w_c g) and in x (dL/dx_a = sum_l R_l sum_c dw_c/dt_a (table row . g_l);
    exactly 0 for a coordinate that is NaN or outside [0, 1], passed at exactly 0 and 1 as th.clamp does); the cell and the hash
    are constants.  n_rows follows mlp_rows' rule (None, or an integer tensor of one element on x's device -- what
    PackedSlots.n_used is): rows r >= min(max(n_rows, 0), N) are NOT READ, give exact zeros in y and dL_dx and add nothing to
    dL_dtable.  Plain torch, any device, any float dtype: the model hashgrid_rows_fused is tested against."""
    _hashgrid_arguments("hashgrid_rows", x, table, spec, n_rows)
    zero = th.zeros((), dtype=x.dtype, device=x.device)
    mask = None
    if n_rows is not None:
        mask = (th.arange(x.shape[0], device=x.device) < n_rows.reshape(1).clamp(min=0)).unsqueeze(1)
        x = th.where(mask, x, zero)
    u = th.where(th.isnan(x), zero, x).clamp(0, 1)
    F, T = spec.features, 1 << spec.log2_table_size
    out = []
    for l, R in enumerate(spec.resolutions):
        p = u * R
        i = p.detach().floor().clamp(max=R - 1).clamp(min=0)
        t = p - i
        i = i.long()
        dense = spec.sizes[l] == (R + 1) ** 3 and (R + 1) ** 3 <= T
        acc = 0
        for c in range(8):
            cx, cy, cz = c & 1, (c >> 1) & 1, (c >> 2) & 1
            ix, iy, iz = i[:, 0] + cx, i[:, 1] + cy, i[:, 2] + cz
            if dense:
                row = (ix + (R + 1) * (iy + (R + 1) * iz)).clamp(max=spec.sizes[l] - 1)
            else:
                row = (((ix * HASH_PRIMES[0]) & 0xffffffff) ^ ((iy * HASH_PRIMES[1]) & 0xffffffff) ^ ((iz * HASH_PRIMES[2]) & 0xffffffff)) & (T - 1)
            wx = t[:, 0] if cx else 1 - t[:, 0]
            wy = t[:, 1] if cy else 1 - t[:, 1]
            wz = t[:, 2] if cz else 1 - t[:, 2]
            acc = acc + ((wx * wy) * wz).unsqueeze(1) * table[spec.offsets[l] + row].to(x.dtype)
        out.append(acc)
    y = th.cat(out, dim=1)
    return y if mask is None else th.where(mask, y, zero)


class _HashGridRowsFn(th.autograd.Function):
    """hashgrid_rows_fused over _C.hashgrid_rows / _C.hashgrid_rows_backward.  Arguments: x, table, n_rows (a tensor or None),
    the spec.  Only x, table and n_rows are saved."""

    @staticmethod
    def forward(ctx, x, table, n_rows, spec):
        y = _fused_kernels("hashgrid_rows").hashgrid_rows(x, table, list(spec.resolutions), spec.log2_table_size, n_rows)
        ctx.spec = spec
        _save_optional(ctx, x, table, n_rows)
        ctx.set_materialize_grads(False)  # an output the loss does not use arrives as None, and goes down as None: no launch
        return y

    @staticmethod
    def backward(ctx, grad_y):
        need_x, need_table = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if grad_y is None or not (need_x or need_table):
            return None, None, None, None
        x, table, n_rows = _saved_optional(ctx)
        dx, dtable = _fused_kernels("hashgrid_rows").hashgrid_rows_backward(x, table, list(ctx.spec.resolutions), ctx.spec.log2_table_size,
                                                                            n_rows, grad_y.contiguous(), need_x, need_table)
        return dx, dtable, None, None


def hashgrid_rows_fused(x: th.Tensor, table: th.Tensor, spec: HashGridSpec, n_rows: Optional[th.Tensor] = None) -> th.Tensor:
    """hashgrid_rows(...) as one HIP kernel, and one for its backward (plus the one that zeroes dL_dtable): a lane owns a row and
    walks the levels; the forward stores y through an LDS transpose; the backward's dL/dx recomputes the eight table rows of
    every level (a plain store per row), and its dL/dtable sums on chip what shares a table row -- the lanes of a wave, then a
    per-workgroup LDS table of f64 cells -- before float atomics leave (so dL_dtable depends on the order of summation in its
    last bits).  The same y, the same n_rows rule (read on the device: no host wait, capturable), each gradient computed only
    when autograd asks for it; autograd keeps x, table and n_rows, nothing else.  N < 2^31 (ValueError).  HIP float32 tensors on
    one device only (n_rows int32 [1]), made contiguous if they are not: anything else is a TypeError -- hashgrid_rows is the
    torch path for it; nothing falls back silently.  Refused in this order: an older binding, the shapes (as hashgrid_rows), N,
    the dtypes, the devices."""
    name, torch_path = "hashgrid_rows_fused", "fragments.hashgrid_rows is the torch path for anything else"
    _fused_kernels("hashgrid_rows")
    _hashgrid_arguments(name, x, table, spec, n_rows)
    _check_row_tensors(name, torch_path, x, [("x", x), ("table", table)], [("n_rows", n_rows)])
    return _HashGridRowsFn.apply(x, table, None if n_rows is None else n_rows.reshape(1), spec)


class HashGrid(th.nn.Module):
    """A multiresolution hash grid as a Module that owns its `table` (a Parameter [spec.offsets[L], F], initialised uniform in
    +-1e-4, tiny-cuda-nn's choice -- not derived here): the learned volumetric field in front of a RowMLP.  Takes hashgrid_spec's
    five numbers and the box lo, hi (3 floats each; default the unit cube).  .spec is the layout, .out_features = L * F.
    forward(x, n_rows=None) maps (x - lo) / (hi - lo) in torch and runs hashgrid_rows_fused on HIP float32 rows and hashgrid_rows
    on anything else."""

    def __init__(self, n_levels: int = 16, features: int = 2, log2_table_size: int = 19, base_resolution: int = 16,
                 per_level_scale: float = 1.38, lo: Sequence[float] = (0.0, 0.0, 0.0), hi: Sequence[float] = (1.0, 1.0, 1.0)):
        super().__init__()
        self.spec = hashgrid_spec(n_levels, features, log2_table_size, base_resolution, per_level_scale)
        self.out_features = len(self.spec.resolutions) * self.spec.features
        lo, hi = th.as_tensor(lo, dtype=th.float32).reshape(-1), th.as_tensor(hi, dtype=th.float32).reshape(-1)
        if lo.numel() != 3 or hi.numel() != 3 or not bool((hi > lo).all()):
            raise ValueError(f"HashGrid: lo and hi must hold 3 floats each with lo < hi, got {lo.tolist()}, {hi.tolist()}")
        self.register_buffer("lo", lo.clone())
        self.register_buffer("hi", hi.clone())
        self.table = th.nn.Parameter(th.empty(self.spec.offsets[-1], self.spec.features).uniform_(-1e-4, 1e-4))

    def forward(self, x: th.Tensor, n_rows: Optional[th.Tensor] = None) -> th.Tensor:
        u = (x - self.lo.to(x.dtype)) / (self.hi - self.lo).to(x.dtype)
        fused = u.is_cuda and u.dtype == th.float32 and self.table.dtype == th.float32
        return (hashgrid_rows_fused if fused else hashgrid_rows)(u, self.table, self.spec, n_rows)


# ---------------------------------------------------------------------------
# The view direction of packed rows as real spherical harmonics: the MLP's second input beside the hash grid (csrc/dmr_sh.hip)
# ---------------------------------------------------------------------------
SH_MAX_DEGREE = 4      # degree^2 = 1, 4, 9 or 16 channels
SH_MAX_VIEWS = 1024    # DMR_SH_MAX_VIEWS: the rows of `origin`
SH_MIN_LENGTH = 1e-8   # a shorter (or non-finite) |w| gives the zero direction


def packed_row_views(frag, packed: PackedSlots) -> th.Tensor:
    """int32 [N], N = packed.rows: entry r is the view index b of the slot that owns row r of a packed tensor -- a slot (b, k, y, x)
    counts when 0 <= packed.row < N --, and -1 in every row no slot owns (the tail [min(n_used, N), N) under capacity=M).  If two
    slots claim one row (a `packed` made for other lists) the entry is one of their views.  Nothing is differentiable; frag.bary
    is not read.  Plain torch, any device: the model packed_row_views_fused is tested against."""
    B, K, H, W = _check_lists("packed_row_views", frag, False)
    rows = _check_packed("packed_row_views", "", frag, packed)
    row = packed.row
    live = (row >= 0) & (row < rows)
    view = th.arange(B, dtype=th.int32, device=row.device).view(B, 1, 1, 1).expand(B, K, H, W)
    out = th.full((rows,), -1, dtype=th.int32, device=row.device)
    out[row[live].long()] = view[live]
    return out


def packed_row_views_fused(frag, packed: PackedSlots) -> th.Tensor:
    """packed_row_views(...) as two stream-ordered HIP launches (a fill with -1, one walk of the slots on the packed unit's lanes
    that writes 4 bytes per counting slot): the same int32 [N], exactly, for a `packed` whose rows have one owner each.  No host
    wait, capturable.  N == 0 or an empty image launches nothing.  K <= 32, B K H W < 2^31 (ValueError).  HIP int32 lists only:
    anything else is a TypeError -- packed_row_views is the torch path for it; nothing falls back silently."""
    name, torch_path = "packed_row_views_fused", "fragments.packed_row_views is the torch path for anything else"
    c = _fused_kernels("packed_row_views")
    B, K, H, W = _check_lists(name, frag, False)
    rows = _check_packed(name, torch_path, frag, packed)
    if B * K * H * W >= 2 ** 31 or rows >= 2 ** 31:
        raise ValueError(f"{name}: B K H W and packed.rows must be below 2^31, got {B * K * H * W} slots, {rows} rows")
    _check_tensors(name, torch_path, frag.pix_to_face, [("packed.row", packed.row)], [])
    return c.packed_row_views(packed.row, rows)


def _sh_arguments(name: str, x, degree, origin, row_view, n_rows) -> int:
    """What sh_rows and sh_rows_fused both refuse (ValueError), in this order: x [N,3], degree, origin [B,3] and B, row_view
    without origin, row_view [N], origin of several views without row_view, n_rows.  -> B (0 without origin)"""
    if x.dim() != 2 or x.shape[1] != 3:
        raise ValueError(f"{name}: x must be [N,3], got {tuple(x.shape)}")
    if isinstance(degree, bool) or not isinstance(degree, int) or not 1 <= degree <= SH_MAX_DEGREE:
        raise ValueError(f"{name}: degree must be an int in 1..{SH_MAX_DEGREE}, got {degree!r}")
    B = 0
    if origin is not None:
        if origin.dim() != 2 or origin.shape[1] != 3:
            raise ValueError(f"{name}: origin must be [B,3], got {tuple(origin.shape)}")
        B = origin.shape[0]
        if not 1 <= B <= SH_MAX_VIEWS:
            raise ValueError(f"{name}: origin must hold 1..{SH_MAX_VIEWS} views, got {B}")
    if row_view is not None:
        if origin is None:
            raise ValueError(f"{name}: row_view needs origin (with origin=None x holds the directions themselves)")
        if tuple(row_view.shape) != (x.shape[0],):
            raise ValueError(f"{name}: row_view must be [N] = {(x.shape[0],)}, got {tuple(row_view.shape)}")
    elif B > 1:
        raise ValueError(f"{name}: origin holds {B} views: row_view must tell the view of every row (packed_row_views_fused)")
    _check_n_rows(name, n_rows)
    return B


def _sh_polynomials(d: th.Tensor, degree: int) -> th.Tensor:
    """[N, degree^2]: channel l*l + l + m is the real spherical harmonic Y_lm of d [N,3] in the Condon-Shortley sign convention,
    written as a homogeneous polynomial of d = (x, y, z) -- the table of include/dmesh_renderer_amd_sh.h."""
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    out = [x * 0 + 0.28209479177387814]   # (d is finite; the product keeps the constant in the graph: its gradient is an exact 0)
    if degree >= 2:
        out += [-0.4886025119029199 * y, 0.4886025119029199 * z, -0.4886025119029199 * x]
    if degree >= 3:
        xx, yy, zz = x * x, y * y, z * z
        out += [1.0925484305920792 * (x * y), -1.0925484305920792 * (y * z), 0.31539156525252005 * (2 * zz - xx - yy),
                -1.0925484305920792 * (x * z), 0.5462742152960396 * (xx - yy)]
    if degree >= 4:
        out += [-0.5900435899266435 * y * (3 * xx - yy), 2.890611442640554 * (x * y) * z, -0.4570457994644658 * y * (4 * zz - xx - yy),
                0.3731763325901154 * z * (2 * zz - 3 * xx - 3 * yy), -0.4570457994644658 * x * (4 * zz - xx - yy),
                1.445305721320277 * z * (xx - yy), -0.5900435899266435 * x * (xx - 3 * yy)]
    return th.stack(out, dim=1)


def _sh_directions(x, origin, row_view, n_rows):
    """(d [N,3], live bool [N]) of sh_rows: the unit vectors (zeros where the length is not finite or below SH_MIN_LENGTH, and in
    rows that are not read) and the rows that are read.  What is masked out is masked BEFORE it is used: a NaN there reaches
    neither d nor a gradient."""
    N = x.shape[0]
    zero = th.zeros((), dtype=x.dtype, device=x.device)
    live = th.ones(N, dtype=th.bool, device=x.device)
    if n_rows is not None:
        live = live & (th.arange(N, device=x.device) < n_rows.reshape(1).clamp(min=0))
    w = x
    if origin is not None:
        if row_view is not None:
            v = row_view.long()
            live = live & (v >= 0) & (v < origin.shape[0])
            o = origin.to(x.dtype)[v.clamp(0, origin.shape[0] - 1)]
        else:
            o = origin.to(x.dtype)[0].unsqueeze(0).expand(N, 3)
        w = th.where(live.unsqueeze(1), x, zero) - th.where(live.unsqueeze(1), o, zero)
    else:
        w = th.where(live.unsqueeze(1), x, zero)
    n = th.sqrt((w.detach() * w.detach()).sum(1))
    ok = live & th.isfinite(n) & ~(n < SH_MIN_LENGTH)
    unit = th.zeros(3, dtype=x.dtype, device=x.device)
    unit[2] = 1
    safe = th.where(ok.unsqueeze(1), w, unit)     # (the rows that are not ok leave here: their gradient is an exact 0)
    d = safe / th.sqrt((safe * safe).sum(1, keepdim=True))
    return th.where(ok.unsqueeze(1), d, zero), live


def sh_rows(x: th.Tensor, degree: int, *, origin: Optional[th.Tensor] = None, row_view: Optional[th.Tensor] = None,
            n_rows: Optional[th.Tensor] = None) -> th.Tensor:
    """The view direction of rows x [N,3] as real spherical harmonics -> [N, degree^2], degree 1..4.  Per row r:
        v = row_view[r] (an integer tensor [N]; without it v = 0)
        w = x[r] - origin[v] with origin [B,3], 1 <= B <= 1024 -- or w = x[r] with origin=None: the caller hands over directions
            (row_view must then be None; an origin of B > 1 views needs row_view)
        n = sqrt(w . w) in x's dtype, d = w / n -- d = (0, 0, 0) if n is not finite or n < 1e-8: dL/dx of the row is then an exact
            0 and it adds nothing to dL/dorigin
        y[r, l*l + l + m] = Y_lm(d), Condon-Shortley signs, homogeneous polynomials of d (tiny-cuda-nn's and the Gaussian-splatting
            code's basis; the table is in include/dmesh_renderer_amd_sh.h)
    NOT READ -- a NaN there reaches nothing; exact zeros in y and dL/dx, nothing added to dL/dorigin -- are a row whose v lies
    outside [0, B) (-1 is what packed_row_views gives a row no slot owns) and a row at or past min(max(n_rows, 0), N), mlp_rows'
    rule (n_rows: None, or an integer tensor of one element on x's device -- what PackedSlots.n_used is).  A row that is read and
    has d = 0 gives (0.2820..., 0, ..., 0).  Differentiable in x and origin: dL/dw = (gd - d (d . gd)) / n with gd = sum_i g_i
    dY_i/dd, dL/dx = dL/dw, dL/dorigin[v] = - the sum over the rows of v.  Plain torch, any device, any float dtype: the model
    sh_rows_fused is tested against."""
    _sh_arguments("sh_rows", x, degree, origin, row_view, n_rows)
    d, live = _sh_directions(x, origin, row_view, n_rows)
    y = _sh_polynomials(d, degree)
    return th.where(live.unsqueeze(1), y, th.zeros((), dtype=y.dtype, device=y.device))


class _ShRowsFn(th.autograd.Function):
    """sh_rows_fused over _C.sh_rows / _C.sh_rows_backward.  Arguments: x, origin, row_view, n_rows (tensors or None), degree.
    Only those tensors are saved: nothing of size [N, degree^2]; the backward recomputes d."""

    @staticmethod
    def forward(ctx, x, origin, row_view, n_rows, degree):
        y = _fused_kernels("sh_rows").sh_rows(x, degree, origin, row_view, n_rows)
        ctx.degree = degree
        _save_optional(ctx, x, origin, row_view, n_rows)
        ctx.set_materialize_grads(False)  # an output the loss does not use arrives as None, and goes down as None: no launch
        return y

    @staticmethod
    def backward(ctx, grad_y):
        need_x, need_origin = ctx.needs_input_grad[0], ctx.saved_mask[1] and ctx.needs_input_grad[1]
        if grad_y is None or not (need_x or need_origin):
            return None, None, None, None, None
        x, origin, row_view, n_rows = _saved_optional(ctx)
        dx, dorigin = _fused_kernels("sh_rows").sh_rows_backward(x, ctx.degree, origin, row_view, n_rows, grad_y.contiguous(), need_x, need_origin)
        return dx, dorigin, None, None, None


def sh_rows_fused(x: th.Tensor, degree: int, *, origin: Optional[th.Tensor] = None, row_view: Optional[th.Tensor] = None,
                  n_rows: Optional[th.Tensor] = None) -> th.Tensor:
    """sh_rows(...) as one HIP kernel, and one for its backward (plus the one that zeroes dL_dorigin): a lane owns a row, `degree`
    is a template parameter, y leaves through an LDS transpose at degree 3 and 4 (row by row below; the upstream arrives row by row).
    The same y, the same rows not read (n_rows and row_view are read on the device: no host wait, capturable), each gradient
    computed only when autograd asks for it; autograd keeps x, origin, row_view and n_rows, nothing of size [N, degree^2].
    dL_dorigin sums a wave's rows with DPP, then per workgroup in an LDS table of f64 cells, before one float atomic per cell
    leaves -- so it depends on the order of summation in its last bits; y and dL_dx do not.  N < 2^31 (ValueError).  HIP float32
    tensors on one device only (row_view int32 [N], n_rows int32 [1]), made contiguous if they are not: anything else is a
    TypeError -- sh_rows is the torch path for it; nothing falls back silently.  Refused in this order: an older binding, the
    arguments (as sh_rows), N, the dtypes, the devices."""
    name, torch_path = "sh_rows_fused", "fragments.sh_rows is the torch path for anything else"
    _fused_kernels("sh_rows")
    _sh_arguments(name, x, degree, origin, row_view, n_rows)
    _check_row_tensors(name, torch_path, x, [("x", x), ("origin", origin)], [("row_view", row_view), ("n_rows", n_rows)])
    return _ShRowsFn.apply(x, origin, row_view, None if n_rows is None else n_rows.reshape(1), degree)


def camera_origins(mv_mats: th.Tensor) -> th.Tensor:
    """[B,3]: the camera centre of every view, from the Modules' mv_mats [B,4,4] (what TriRenderer / TetRenderer.forward take):
    the translation column of the inverse, inv(mv_mats)[:, :3, 3] -- the Modules hand mv_mats.transpose(1, 2) and its inverse
    down, and the kernels read a pixel ray's origin at inv_mv[12..14] of that storage, which is this column.  Plain torch through
    th.linalg.inv, so it is differentiable: dL/dorigin reaches mv_mats (pose refinement)."""
    if mv_mats.dim() != 3 or tuple(mv_mats.shape[1:]) != (4, 4):
        raise ValueError(f"camera_origins: mv_mats must be [B,4,4], got {tuple(mv_mats.shape)}")
    return th.linalg.inv(mv_mats)[:, :3, 3]


class ViewSH(th.nn.Module):
    """The spherical-harmonics encoding of the view direction as a Module without parameters: .degree, .out_features =
    degree^2.  forward(x, origin=None, row_view=None, n_rows=None) runs sh_rows_fused on HIP float32 rows and sh_rows on
    anything else, as HashGrid does."""

    def __init__(self, degree: int = 4):
        super().__init__()
        if isinstance(degree, bool) or not isinstance(degree, int) or not 1 <= degree <= SH_MAX_DEGREE:
            raise ValueError(f"ViewSH: degree must be an int in 1..{SH_MAX_DEGREE}, got {degree!r}")
        self.degree = degree
        self.out_features = degree * degree

    def forward(self, x: th.Tensor, origin: Optional[th.Tensor] = None, row_view: Optional[th.Tensor] = None,
                n_rows: Optional[th.Tensor] = None) -> th.Tensor:
        fused = x.is_cuda and x.dtype == th.float32 and (origin is None or origin.dtype == th.float32)
        return (sh_rows_fused if fused else sh_rows)(x, self.degree, origin=origin, row_view=row_view, n_rows=n_rows)


# ---------------------------------------------------------------------------
# Direction rows looked up in a learnable lat-long environment map: the background, and a specular term (csrc/dmr_envmap.hip)
# ---------------------------------------------------------------------------
ENVMAP_MAX_CHANNELS = 16     # DMR_ENVMAP_MAX_CHANNELS
ENVMAP_MIN_LENGTH = 1e-8     # a shorter (or non-finite) |d| is a skipped row
ENVMAP_POLE_RHO2 = 1e-12     # ux^2 + uy^2 below it: phi = 0, and the row's dL/dd is an exact 0


def _envmap_arguments(name: str, d, envmap, n_rows):
    """What envmap_rows and envmap_rows_fused both refuse (ValueError), in this order: d [N,3], envmap [He,We,C], C, an empty map,
    a map too large for the kernels' keys, n_rows."""
    if d.dim() != 2 or d.shape[1] != 3:
        raise ValueError(f"{name}: d must be [N,3], got {tuple(d.shape)}")
    if envmap.dim() != 3:
        raise ValueError(f"{name}: envmap must be [He,We,C], got {tuple(envmap.shape)}")
    He, We, C = envmap.shape
    if not 1 <= C <= ENVMAP_MAX_CHANNELS:
        raise ValueError(f"{name}: C must be in 1..{ENVMAP_MAX_CHANNELS}, got {C}")
    if He < 1 or We < 1:
        raise ValueError(f"{name}: the map must have at least one texel, got {tuple(envmap.shape)}")
    if He * We * ((C + 3) // 4) >= 2 ** 31:
        raise ValueError(f"{name}: He * We * ceil(C / 4) must be below 2^31, got {tuple(envmap.shape)}")
    _check_n_rows(name, n_rows)


def envmap_rows(d: th.Tensor, envmap: th.Tensor, *, n_rows: Optional[th.Tensor] = None) -> th.Tensor:
    """Direction rows d [N,3] looked up in a lat-long (equirectangular) map envmap [He,We,C], channel-last like composite_texture's
    texture, 1 <= C <= 16 -> [N,C].  Per row r, in d's dtype:
        n = sqrt(d . d); the row is SKIPPED when n is not finite or n < 1e-8, or when r >= min(max(n_rows, 0), N), mlp_rows' rule
            (n_rows: None, or an integer tensor of one element on d's device -- what PackedSlots.n_used is): it is not read -- a
            NaN there reaches nothing --, gives exact zeros in y and dL/dd and adds nothing to dL/denvmap
        u = d / n, rho2 = ux^2 + uy^2; the pole axis is z, as in sh_rows' table: theta = acos(clamp(uz, -1, 1)), evaluated as
            atan2(sqrt(rho2), uz) (the same angle, without acos' loss of digits next to the poles), phi = atan2(uy, ux) -- where
            rho2 < 1e-12: phi = 0, and the row's dL/dd is an exact 0
        s = phi / (2 pi) + 0.5, t = theta / pi: row 0 of the map is +z, +x the middle of a row
        x = s We - 0.5, y = t He - 0.5 (texel centres at half-integers, composite_texture's rule); x0 = floor(x), fx = x - x0 from
            the unwrapped coordinate, likewise y; columns repeat, rows clamp
        y[r] = the bilinear mix of the four texels.
    Differentiable in d and envmap: dL/denvmap is the four weights times the upstream, summed over the rows; dL/dd goes through
    (x, y), (phi, theta) and the normalisation, the cell (the floors) held constant as in composite_texture.  In float32 the
    coordinates carry the rounding of the two atan2 times the map's size: the deviation from float64 grows with He and We.
    Not modelled: mip levels (envmap_lod_rows looks up a pyramid of this map), cube maps, a map per view, a nearest filter.
    Plain torch, any device, any float dtype: the model envmap_rows_fused is tested against."""
    _envmap_arguments("envmap_rows", d, envmap, n_rows)
    N, (He, We, C) = d.shape[0], envmap.shape
    zero = th.zeros((), dtype=d.dtype, device=d.device)
    live = th.ones(N, dtype=th.bool, device=d.device)
    if n_rows is not None:
        live = live & (th.arange(N, device=d.device) < n_rows.reshape(1).clamp(min=0))
    w = th.where(live.unsqueeze(1), d, zero)
    n = th.sqrt((w.detach() * w.detach()).sum(1))
    ok = live & th.isfinite(n) & ~(n < ENVMAP_MIN_LENGTH)
    ex = th.zeros(3, dtype=d.dtype, device=d.device)
    ex[0] = 1
    safe = th.where(ok.unsqueeze(1), w, ex)        # (the rows that are not ok leave here: their gradient is an exact 0)
    u = safe / th.sqrt((safe * safe).sum(1, keepdim=True))
    pole = (u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1]).detach() < ENVMAP_POLE_RHO2
    us = th.where(pole.unsqueeze(1), ex, u)        # (... and the poles here)
    rho = th.sqrt(us[:, 0] * us[:, 0] + us[:, 1] * us[:, 1])
    phi = th.atan2(us[:, 1], us[:, 0])
    theta = th.atan2(rho, us[:, 2])
    theta = th.where(pole, th.where(u[:, 2].detach() > 0, zero, zero + math.pi), theta)
    x = (phi / (2 * math.pi) + 0.5) * We - 0.5
    y = (theta / math.pi) * He - 0.5
    x0, y0 = x.detach().floor(), y.detach().floor()
    fx, fy = (x - x0).unsqueeze(1), (y - y0).unsqueeze(1)
    ix0, ix1 = _wrap_index(x0.long(), We, "repeat"), _wrap_index(x0.long() + 1, We, "repeat")
    iy0, iy1 = _wrap_index(y0.long(), He, "clamp"), _wrap_index(y0.long() + 1, He, "clamp")
    e = envmap.to(d.dtype)
    out = (1 - fy) * ((1 - fx) * e[iy0, ix0] + fx * e[iy0, ix1]) + fy * ((1 - fx) * e[iy1, ix0] + fx * e[iy1, ix1])
    return th.where(ok.unsqueeze(1), out, zero)


class _EnvMapRowsFn(th.autograd.Function):
    """envmap_rows_fused over _C.envmap_rows / _C.envmap_rows_backward.  Arguments: d, envmap, n_rows (a tensor or None).  Only
    those are saved: nothing of size [N,C]; the backward re-reads the four texels."""

    @staticmethod
    def forward(ctx, d, envmap, n_rows):
        y = _fused_kernels("envmap_rows").envmap_rows(d, envmap, n_rows)
        _save_optional(ctx, d, envmap, n_rows)
        ctx.set_materialize_grads(False)  # an output the loss does not use arrives as None, and goes down as None: no launch
        return y

    @staticmethod
    def backward(ctx, grad_y):
        need_d, need_envmap = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if grad_y is None or not (need_d or need_envmap):
            return None, None, None
        d, envmap, n_rows = _saved_optional(ctx)
        dd, denvmap = _fused_kernels("envmap_rows").envmap_rows_backward(d, envmap, n_rows, grad_y.contiguous(), need_d, need_envmap)
        return dd, denvmap, None


def envmap_rows_fused(d: th.Tensor, envmap: th.Tensor, *, n_rows: Optional[th.Tensor] = None) -> th.Tensor:
    """envmap_rows(...) as one HIP kernel, and one for its backward (plus the one that zeroes dL_denvmap): a lane owns a row, forms
    its four texel addresses and weights once and takes the channels in chunks of four (float4 texel reads when C % 4 == 0); y
    leaves row by row or through an LDS transpose, per C the shape that measured faster.  The backward's dL/dd re-reads the four
    texels (a plain store per row, no atomics); its dL/denvmap sums on chip what shares a texel -- the lanes of a wave, then a
    per-workgroup LDS table of f64 cells -- before float atomics leave (so dL_denvmap depends on the order of summation in its
    last bits; y and dL_dd do not).  The same y, the same skipped rows (n_rows is read on the device: no host wait, capturable),
    each gradient computed only when autograd asks for it; autograd keeps d, envmap and n_rows, nothing of size [N,C].  Whatever
    the bits of d, every access is in bounds.  N < 2^31 (ValueError).  HIP float32 tensors on one device only (n_rows int32 [1]),
    made contiguous if they are not: anything else is a TypeError -- envmap_rows is the torch path for it; nothing falls back
    silently.  Refused in this order: an older binding, the arguments (as envmap_rows), N, the dtypes, the devices."""
    name, torch_path = "envmap_rows_fused", "fragments.envmap_rows is the torch path for anything else"
    _fused_kernels("envmap_rows")
    _envmap_arguments(name, d, envmap, n_rows)
    _check_row_tensors(name, torch_path, d, [("d", d), ("envmap", envmap)], [("n_rows", n_rows)])
    return _EnvMapRowsFn.apply(d, envmap, None if n_rows is None else n_rows.reshape(1))


class EnvMap(th.nn.Module):
    """A lat-long environment map as a Module that owns its `envmap` (a Parameter [height, width, channels], initialised to 0.5:
    mid-grey, not derived here): the learnable background behind the faces, or a specular term over packed rows.
    frame (optional, [3,3]): d is rotated to frame @ d in torch before the lookup, for a pole axis other than z -- its rows are
    the map's x, y and z axes in world coordinates; kept as a buffer.  .out_features = channels.
    forward(d, n_rows=None) runs envmap_rows_fused on HIP float32 rows and envmap_rows on anything else, as HashGrid does."""

    def __init__(self, height: int, width: int, channels: int = 3, frame: Optional[th.Tensor] = None):
        super().__init__()
        for what, v in (("height", height), ("width", width)):
            if isinstance(v, bool) or not isinstance(v, int) or v < 1:
                raise ValueError(f"EnvMap: {what} must be a positive int, got {v!r}")
        if isinstance(channels, bool) or not isinstance(channels, int) or not 1 <= channels <= ENVMAP_MAX_CHANNELS:
            raise ValueError(f"EnvMap: channels must be an int in 1..{ENVMAP_MAX_CHANNELS}, got {channels!r}")
        if frame is not None:
            frame = th.as_tensor(frame, dtype=th.float32)
            if tuple(frame.shape) != (3, 3):
                raise ValueError(f"EnvMap: frame must be [3,3], got {tuple(frame.shape)}")
            frame = frame.clone()
        self.register_buffer("frame", frame)
        self.out_features = channels
        self.envmap = th.nn.Parameter(th.full((height, width, channels), 0.5))

    def forward(self, d: th.Tensor, n_rows: Optional[th.Tensor] = None) -> th.Tensor:
        if self.frame is not None:
            d = d @ self.frame.to(d.dtype).T
        fused = d.is_cuda and d.dtype == th.float32 and self.envmap.dtype == th.float32
        return (envmap_rows_fused if fused else envmap_rows)(d, self.envmap, n_rows=n_rows)


# ---------------------------------------------------------------------------
# A mip pyramid of that map, looked up at a per-row level of detail: the specular term of a rough surface (csrc/dmr_envmap_lod.hip)
# ---------------------------------------------------------------------------
ENVMAP_LOD_MAX_LEVELS = 12   # DMR_ENVMAP_LOD_MAX_LEVELS


def _pyramid_spec(name: str, He, We, L, C) -> Tuple[list, int]:
    """THE LAYOUT of a pyramid (include/dmesh_renderer_amd_envmap_lod.h), restated: the spec is (He, We, L), 1 <= L <= 12; level l
    has He >> l rows and We >> l columns, He and We multiples of 2^(L-1); pyramid [T,C] holds level l as the row-major
    [He_l, We_l, C] block that starts at row off_l = sum_{j<l} He_j We_j; level 0 is the base map.  What every function here
    refuses of a spec (ValueError), in this order: C, L, an empty map, the multiples, a pyramid too large for the kernels' keys.
    -> ([off_0, ..., off_{L-1}], T)"""
    if not 1 <= C <= ENVMAP_MAX_CHANNELS:
        raise ValueError(f"{name}: C must be in 1..{ENVMAP_MAX_CHANNELS}, got {C}")
    if any(isinstance(v, bool) or not isinstance(v, int) for v in (He, We, L)) or not 1 <= L <= ENVMAP_LOD_MAX_LEVELS:
        raise ValueError(f"{name}: levels must be an int in 1..{ENVMAP_LOD_MAX_LEVELS} (the spec: ints (He, We, L)), got {(He, We, L)!r}")
    if He < 1 or We < 1:
        raise ValueError(f"{name}: the map must have at least one texel, got {(He, We)}")
    if He % (1 << (L - 1)) or We % (1 << (L - 1)):
        raise ValueError(f"{name}: He and We must be multiples of 2^(levels-1) = {1 << (L - 1)}, got {(He, We)}")
    offs, T = [], 0
    for l in range(L):
        offs.append(T)
        T += (He >> l) * (We >> l)
    if T * ((C + 3) // 4) >= 2 ** 31:
        raise ValueError(f"{name}: T * ceil(C / 4) must be below 2^31, got T = {T}, C = {C}")
    return offs, T


def _pyramid_arguments(name: str, envmap, levels):
    """What envmap_pyramid and envmap_pyramid_fused both refuse (ValueError): envmap [He,We,C], then the spec (_pyramid_spec)."""
    if envmap.dim() != 3:
        raise ValueError(f"{name}: envmap must be [He,We,C], got {tuple(envmap.shape)}")
    He, We, C = envmap.shape
    return _pyramid_spec(name, He, We, levels, C)


def envmap_pyramid(envmap: th.Tensor, levels: int) -> th.Tensor:
    """The mip pyramid of a lat-long map envmap [He,We,C] -> [T,C] in _pyramid_spec's layout, `levels` = L of them: level 0 is
    the map itself, level l+1 at (i, j) is
        ((a + b) + (c + d)) * 0.25,   a, b = level l at (2i, 2j), (2i, 2j+1);  c, d = the same columns of row 2i+1
    -- this order of summation is part of the contract: envmap_pyramid_fused equals it bit for bit.  A BOX mip chain in the map's
    own parameterisation, NOT a solid-angle or GGX prefilter; envmap_lod_rows accepts any [T,C] tensor in this layout, so a caller
    may pass a pyramid prefiltered elsewhere.  Differentiable in envmap.  Plain torch, any device, any float dtype."""
    _pyramid_arguments("envmap_pyramid", envmap, levels)
    C = envmap.shape[2]
    out, cur = [envmap.reshape(-1, C)], envmap
    for _ in range(levels - 1):
        cur = ((cur[0::2, 0::2] + cur[0::2, 1::2]) + (cur[1::2, 0::2] + cur[1::2, 1::2])) * 0.25
        out.append(cur.reshape(-1, C))
    return th.cat(out, 0)


class _EnvMapPyramidFn(th.autograd.Function):
    """envmap_pyramid_fused over _C.envmap_pyramid / _C.envmap_pyramid_backward.  Arguments: envmap, levels.  Nothing is saved."""

    @staticmethod
    def forward(ctx, envmap, levels):
        ctx.spec = (envmap.shape[0], envmap.shape[1], levels)
        ctx.set_materialize_grads(False)
        return _fused_kernels("envmap_pyramid").envmap_pyramid(envmap, levels)

    @staticmethod
    def backward(ctx, grad_pyramid):
        if grad_pyramid is None or not ctx.needs_input_grad[0]:
            return None, None
        return _fused_kernels("envmap_pyramid").envmap_pyramid_backward(grad_pyramid.contiguous(), *ctx.spec), None


def envmap_pyramid_fused(envmap: th.Tensor, levels: int) -> th.Tensor:
    """envmap_pyramid(...) on HIP: one small launch per level, each reading the level below, and for the backward one gather
    launch without atomics -- per base texel (y, x) Horner from the coarsest level down, acc = g_l[y >> l, x >> l] + 0.25 acc.
    Multiplying by 0.25 is exact: both directions equal envmap_pyramid in float32 bit for bit on finite, normal values.  A HIP
    float32 tensor only (made contiguous if it is not): anything else is a TypeError -- envmap_pyramid is the torch path for it;
    nothing falls back silently.  Refused in this order: an older binding, the arguments (as envmap_pyramid), the dtype, the device."""
    name, torch_path = "envmap_pyramid_fused", "fragments.envmap_pyramid is the torch path for anything else"
    _fused_kernels("envmap_pyramid")
    _pyramid_arguments(name, envmap, levels)
    _check_row_tensors(name, torch_path, envmap, [("envmap", envmap)], [])
    return _EnvMapPyramidFn.apply(envmap, levels)


def _envmap_lod_angles(d, n_rows):
    """(ok [N] bool, phi [N], theta [N]) of direction rows d [N,3], by envmap_rows' own lines (that function stays as it is, the
    model of the single-level unit): ok is False in a skipped row (whose phi and theta are those of +x, with an exact 0 gradient);
    at a pole phi = 0 and both angles are constants."""
    N = d.shape[0]
    zero = th.zeros((), dtype=d.dtype, device=d.device)
    live = th.ones(N, dtype=th.bool, device=d.device)
    if n_rows is not None:
        live = live & (th.arange(N, device=d.device) < n_rows.reshape(1).clamp(min=0))
    w = th.where(live.unsqueeze(1), d, zero)
    n = th.sqrt((w.detach() * w.detach()).sum(1))
    ok = live & th.isfinite(n) & ~(n < ENVMAP_MIN_LENGTH)
    ex = th.zeros(3, dtype=d.dtype, device=d.device)
    ex[0] = 1
    safe = th.where(ok.unsqueeze(1), w, ex)        # (the rows that are not ok leave here: their gradient is an exact 0)
    u = safe / th.sqrt((safe * safe).sum(1, keepdim=True))
    pole = (u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1]).detach() < ENVMAP_POLE_RHO2
    us = th.where(pole.unsqueeze(1), ex, u)        # (... and the poles here)
    rho = th.sqrt(us[:, 0] * us[:, 0] + us[:, 1] * us[:, 1])
    phi = th.atan2(us[:, 1], us[:, 0])
    theta = th.atan2(rho, us[:, 2])
    theta = th.where(pole, th.where(u[:, 2].detach() > 0, zero, zero + math.pi), theta)
    return ok, phi, theta


def _envmap_lod_bilinear(table, off, He, We, phi, theta):
    """[N,C]: envmap_rows' bilinear mix at (phi, theta) [N], per row in the row-major [He,We,C] block of table [T,C] that starts at
    its row `off` -- texel centres at half-integers, the floors from the unwrapped coordinates and held constant, columns repeating
    and rows clamped.  off, He, We: int64 tensors [N] on phi's device (a row's level of the pyramid)."""
    x = (phi / (2 * math.pi) + 0.5) * We.to(phi.dtype) - 0.5
    y = (theta / math.pi) * He.to(phi.dtype) - 0.5
    x0, y0 = x.detach().floor(), y.detach().floor()
    fx, fy = (x - x0).unsqueeze(1), (y - y0).unsqueeze(1)
    ix0, ix1 = th.remainder(x0.long(), We), th.remainder(x0.long() + 1, We)
    iy0, iy1 = th.minimum(y0.long().clamp(min=0), He - 1), th.minimum((y0.long() + 1).clamp(min=0), He - 1)
    r0, r1 = off + iy0 * We, off + iy1 * We
    return (1 - fy) * ((1 - fx) * table[r0 + ix0] + fx * table[r0 + ix1]) + fy * ((1 - fx) * table[r1 + ix0] + fx * table[r1 + ix1])


def _envmap_lod_arguments(name: str, d, lod, pyramid, levels, n_rows):
    """What envmap_lod_rows and envmap_lod_rows_fused both refuse (ValueError), in this order: d [N,3], lod [N] or [N,1], pyramid
    [T,C], levels = (He, We, L), the spec (_pyramid_spec), the pyramid's T, n_rows.  -> ((He, We, L), [off_l])"""
    if d.dim() != 2 or d.shape[1] != 3:
        raise ValueError(f"{name}: d must be [N,3], got {tuple(d.shape)}")
    if tuple(lod.shape) not in ((d.shape[0],), (d.shape[0], 1)):
        raise ValueError(f"{name}: lod must be [N] or [N,1] = {(d.shape[0],)}, got {tuple(lod.shape)}")
    if pyramid.dim() != 2:
        raise ValueError(f"{name}: pyramid must be [T,C], got {tuple(pyramid.shape)}")
    if not isinstance(levels, (tuple, list)) or len(levels) != 3:
        raise ValueError(f"{name}: levels must be the spec (He, We, L), got {levels!r}")
    He, We, L = levels
    offs, T = _pyramid_spec(name, He, We, L, pyramid.shape[1])
    if pyramid.shape[0] != T:
        raise ValueError(f"{name}: pyramid must have the T = {T} rows of the spec {(He, We, L)}, got {tuple(pyramid.shape)}")
    _check_n_rows(name, n_rows)
    return (He, We, L), offs


def envmap_lod_rows(d: th.Tensor, lod: th.Tensor, pyramid: th.Tensor, levels: Tuple[int, int, int], *,
                    n_rows: Optional[th.Tensor] = None) -> th.Tensor:
    """Direction rows d [N,3] looked up in a mip pyramid [T,C] of a lat-long map (envmap_pyramid's layout, levels = (He, We, L))
    at a level of detail per row, lod [N] or [N,1] -> [N,C]: bilinear in two adjacent levels, linear between them.  Per row r:
        n, u, rho2, theta, phi, s, t, the pole rule and the SKIPPED row exactly as envmap_rows states them; a skipped row reads
            neither lod nor the upstream, gives exact zeros in y, dL/dd and dL/dlod and adds nothing to dL/dpyramid
        lam = lod >= 0 ? (lod <= L-1 ? lod : L-1) : 0 (a NaN compares false and becomes 0, +Inf becomes L-1)
        inside = lod > 0 and lod < L-1;  l0 = min(floor(lam), L-2), l1 = l0 + 1, f = lam - l0 in [0, 1];  L == 1: l0 = l1 = 0, f = 0
        B_l = envmap_rows' bilinear mix at level l: its own x = s We_l - 0.5, y = t He_l - 0.5, floors and fractions, columns
            repeating and rows clamped on (We_l, He_l)
        y[r] = (1-f) B_l0 + f B_l1.
    Differentiable in d, lod and pyramid: dL/dlod = (B_l1 - B_l0) . g where inside holds and an exact 0 elsewhere (at an integer
    lod the derivative to the right); dL/dd holds the cell constant at both levels and is an exact 0 at a pole; dL/dpyramid is the
    eight weights times the upstream, summed over the rows.  The level of detail is the caller's mapping (from a roughness, say).
    Not modelled: a GGX or solid-angle prefilter, cube maps, anisotropic footprints, a level from screen-space derivatives.  Plain
    torch, any device, any float dtype: the model envmap_lod_rows_fused is tested against."""
    (He, We, L), offs = _envmap_lod_arguments("envmap_lod_rows", d, lod, pyramid, levels, n_rows)
    ok, phi, theta = _envmap_lod_angles(d, n_rows)
    zero = th.zeros((), dtype=d.dtype, device=d.device)
    lod = th.where(ok, lod.reshape(-1).to(d.dtype), zero)       # (a skipped row's lod leaves here)
    top = float(L - 1)
    lam = th.where(lod >= 0, th.where(lod <= top, lod, zero + top), zero).detach()
    inside = ((lod > 0) & (lod < top)).detach()
    lam = th.where(inside, lod, lam)                            # (the gradient passes where inside holds, and only there)
    l0 = lam.detach().floor().long().clamp(max=L - 2).clamp(min=0)
    l1 = (l0 + 1).clamp(max=L - 1)
    f = (lam - l0.to(d.dtype)).unsqueeze(1)                     # (L == 1: lam = 0 = l0)
    off, hs, ws = (th.tensor(v, dtype=th.int64, device=d.device) for v in (offs, [He >> l for l in range(L)], [We >> l for l in range(L)]))
    table = pyramid.to(d.dtype)
    b0, b1 = (_envmap_lod_bilinear(table, off[l], hs[l], ws[l], phi, theta) for l in (l0, l1))
    return th.where(ok.unsqueeze(1), (1 - f) * b0 + f * b1, zero)


class _EnvMapLodRowsFn(th.autograd.Function):
    """envmap_lod_rows_fused over _C.envmap_lod_rows / _C.envmap_lod_rows_backward.  Arguments: d, lod (as given: [N] or [N,1] at its
    own stride), pyramid, n_rows (a tensor or None), He, We, L.  Only the tensors are saved: nothing of size [N,C]."""

    @staticmethod
    def forward(ctx, d, lod, pyramid, n_rows, He, We, L):
        y = _fused_kernels("envmap_lod_rows").envmap_lod_rows(d, lod, pyramid, He, We, L, n_rows)
        _save_optional(ctx, d, lod, pyramid, n_rows)
        ctx.spec = (He, We, L)
        ctx.set_materialize_grads(False)  # an output the loss does not use arrives as None, and goes down as None: no launch
        return y

    @staticmethod
    def backward(ctx, grad_y):
        need = ctx.needs_input_grad[:3]
        if grad_y is None or not any(need):
            return (None,) * 7
        d, lod, pyramid, n_rows = _saved_optional(ctx)
        dd, dlod, dpyr = _fused_kernels("envmap_lod_rows").envmap_lod_rows_backward(d, lod, pyramid, *ctx.spec, n_rows, grad_y.contiguous(), *need)
        return dd, None if dlod is None else dlod.view(lod.shape), dpyr, None, None, None, None


def envmap_lod_rows_fused(d: th.Tensor, lod: th.Tensor, pyramid: th.Tensor, levels: Tuple[int, int, int], *,
                          n_rows: Optional[th.Tensor] = None) -> th.Tensor:
    """envmap_lod_rows(...) as one HIP kernel, and one for its backward (plus the one that zeroes dL_dpyramid): a lane owns a row,
    evaluates the two atan2, the square root and the normalisation ONCE, forms the eight texel addresses and weights from (s, t) per
    level and takes the channels in chunks of four (float4 texel reads when C % 4 == 0).  The forward does not read a level whose
    weight is exactly 0.  The backward computes each gradient only when autograd asks for it: dL/dd and dL/dlod are plain stores
    per row; dL/dpyramid sums on chip what shares a texel -- the lanes of a wave, then a per-workgroup LDS table of f64 cells --
    before float atomics leave (so it depends on the order of summation in its last bits; y, dL_dd and dL_dlod do not).  lod is
    read in place at its own stride: a column of a wider tensor (out[:, 3] of an MLP's output) needs no copy.  n_rows is read on
    the device: no host wait, capturable.  Whatever the bits of d and lod, every access is in bounds.  N < 2^31 (ValueError).  HIP
    float32 tensors on one device only (n_rows int32 [1]): anything else is a TypeError -- envmap_lod_rows is the torch path for
    it; nothing falls back silently.  Refused in this order: an older binding, the arguments (as envmap_lod_rows), N, the dtypes,
    the devices."""
    name, torch_path = "envmap_lod_rows_fused", "fragments.envmap_lod_rows is the torch path for anything else"
    _fused_kernels("envmap_lod_rows")
    (He, We, L), _ = _envmap_lod_arguments(name, d, lod, pyramid, levels, n_rows)
    _check_row_tensors(name, torch_path, d, [("d", d), ("lod", lod), ("pyramid", pyramid)], [("n_rows", n_rows)])
    return _EnvMapLodRowsFn.apply(d, lod, pyramid, None if n_rows is None else n_rows.reshape(1), He, We, L)


class EnvMapPyramid(th.nn.Module):
    """A lat-long environment map looked up at a per-row level of detail, as a Module that owns the BASE map `envmap` (a Parameter
    [height, width, channels], initialised to 0.5 like EnvMap's) and builds its mip pyramid in every forward: the specular term of
    a rough surface.  levels: L of the pyramid; None: the largest the sizes allow (height and width multiples of 2^(L-1)), up to
    12.  frame: EnvMap's.  .levels = L, .out_features = channels.
    forward(d, lod, n_rows=None) runs envmap_pyramid_fused and envmap_lod_rows_fused on HIP float32 rows and the torch models on
    anything else; the gradient reaches envmap through the pyramid.  lod is the caller's mapping, roughness * (levels - 1), say."""

    def __init__(self, height: int, width: int, channels: int = 3, levels: Optional[int] = None, frame: Optional[th.Tensor] = None):
        super().__init__()
        for what, v in (("height", height), ("width", width)):
            if isinstance(v, bool) or not isinstance(v, int) or v < 1:
                raise ValueError(f"EnvMapPyramid: {what} must be a positive int, got {v!r}")
        if isinstance(channels, bool) or not isinstance(channels, int) or not 1 <= channels <= ENVMAP_MAX_CHANNELS:
            raise ValueError(f"EnvMapPyramid: channels must be an int in 1..{ENVMAP_MAX_CHANNELS}, got {channels!r}")
        if levels is None:
            levels = 1
            while levels < ENVMAP_LOD_MAX_LEVELS and height % (1 << levels) == 0 and width % (1 << levels) == 0:
                levels += 1
        _pyramid_spec("EnvMapPyramid", height, width, levels, channels)
        if frame is not None:
            frame = th.as_tensor(frame, dtype=th.float32)
            if tuple(frame.shape) != (3, 3):
                raise ValueError(f"EnvMapPyramid: frame must be [3,3], got {tuple(frame.shape)}")
            frame = frame.clone()
        self.register_buffer("frame", frame)
        self.out_features, self.levels = channels, levels
        self.envmap = th.nn.Parameter(th.full((height, width, channels), 0.5))

    def forward(self, d: th.Tensor, lod: th.Tensor, n_rows: Optional[th.Tensor] = None) -> th.Tensor:
        if self.frame is not None:
            d = d @ self.frame.to(d.dtype).T
        spec = (self.envmap.shape[0], self.envmap.shape[1], self.levels)
        if d.is_cuda and d.dtype == th.float32 and lod.dtype == th.float32 and self.envmap.dtype == th.float32:
            return envmap_lod_rows_fused(d, lod, envmap_pyramid_fused(self.envmap, self.levels), spec, n_rows=n_rows)
        return envmap_lod_rows(d, lod, envmap_pyramid(self.envmap, self.levels), spec, n_rows=n_rows)


def pixel_directions(mv_mats: th.Tensor, proj_mats: th.Tensor, H: int, W: int) -> th.Tensor:
    """[B,H,W,3]: the normalised world-space ray of every pixel centre, from the Modules' mv_mats and proj_mats [B,4,4] (what
    TriRenderer / TetRenderer.forward take; camera_origins' matrix convention), by the arithmetic of the kernels' pixel ray: the
    pixel (px, py) goes through ndc ((2 (px + 0.5) + 1) / W - 1, (2 (py + 0.5) + 1) / H - 1, -1), that point through inv(proj_mats)
    and the affine part of inv(mv_mats) into world space, w = it - the camera centre, d = w / (|w| + 1e-7) -- the tri renderer's
    length (the tet renderer divides by max(|w|, 1e-4): the same to 1e-7 of |w|).  The tet renderer's seeded jitter of the pixel
    position (seed > 0) is NOT modelled: these are the rays of seed = 0.  Plain torch through th.linalg.inv, any device and float
    dtype, differentiable to both matrices."""
    for what, m in (("mv_mats", mv_mats), ("proj_mats", proj_mats)):
        if m.dim() != 3 or tuple(m.shape[1:]) != (4, 4):
            raise ValueError(f"pixel_directions: {what} must be [B,4,4], got {tuple(m.shape)}")
    if proj_mats.shape[0] != mv_mats.shape[0]:
        raise ValueError(f"pixel_directions: mv_mats and proj_mats must hold the same views, got {mv_mats.shape[0]} and {proj_mats.shape[0]}")
    if isinstance(H, bool) or isinstance(W, bool) or not isinstance(H, int) or not isinstance(W, int) or H < 1 or W < 1:
        raise ValueError(f"pixel_directions: H and W must be positive ints, got {H!r}, {W!r}")
    dt, dev = mv_mats.dtype, mv_mats.device
    im, ip = th.linalg.inv(mv_mats), th.linalg.inv(proj_mats.to(dt))
    nx = ((th.arange(W, dtype=dt, device=dev) + 0.5) * 2 + 1) / W - 1
    ny = ((th.arange(H, dtype=dt, device=dev) + 0.5) * 2 + 1) / H - 1
    ndc = th.stack([nx.view(1, W).expand(H, W), ny.view(H, 1).expand(H, W), -th.ones(H, W, dtype=dt, device=dev),
                    th.ones(H, W, dtype=dt, device=dev)], -1)                       # [H,W,4]
    pv = th.einsum("bij,hwj->bhwi", ip, ndc)                                        # [B,H,W,4]
    w = th.einsum("bij,bhwj->bhwi", im[:, :3, :3], pv[..., :3])                     # (+ the centre, - the centre)
    return w / (th.sqrt((w * w).sum(-1, keepdim=True)) + 1e-7)


# ---------------------------------------------------------------------------
# The surface frame of packed rows: hit point, geometric normal towards the camera, mirrored view ray (csrc/dmr_surface.hip)
# ---------------------------------------------------------------------------
SURFACE_MIN_AREA = 1e-20    # a face whose |e1 x e2| is smaller (or not finite) is degenerate: normal 0
SURFACE_MIN_LENGTH = 1e-8   # SH_MIN_LENGTH: a shorter (or non-finite) |hit - origin| gives the zero direction


class SurfaceRows(NamedTuple):
    """What surface_packed / surface_packed_fused return: three row tensors [N,3], N = packed.rows."""
    hit: th.Tensor       # the point of the face the slot's ray meets: interpolate_packed(frag, packed, faces, verts)
    normal: th.Tensor    # the unit geometric normal of the face, turned towards the camera; 0 on a degenerate face
    reflect: th.Tensor   # the view direction mirrored at the face: unit length; the view direction itself on a degenerate face


def _unit_or_zero(x: th.Tensor, least: float) -> Tuple[th.Tensor, th.Tensor]:
    """(x / |x| along the last axis, ok) -- zeros, and an exact 0 gradient, where |x| is not finite or below `least`."""
    n = th.sqrt((x.detach() * x.detach()).sum(-1))
    ok = (th.isfinite(n) & ~(n < least)).unsqueeze(-1)
    unit = th.zeros(3, dtype=x.dtype, device=x.device)
    unit[2] = 1
    safe = th.where(ok, x, unit)     # (what is not ok leaves here: its gradient is an exact 0)
    return th.where(ok, safe / th.sqrt((safe * safe).sum(-1, keepdim=True)), th.zeros((), dtype=x.dtype, device=x.device)), ok


def _check_surface(name: str, frag, packed, faces, verts, origin) -> int:
    """The shapes surface_packed and surface_packed_fused both refuse (ValueError) -> packed.rows."""
    B, K, H, W = _check_lists(name, frag, True)
    if faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"{name}: faces must be [F,3], got {tuple(faces.shape)}")
    if verts.dim() != 2 or verts.shape[1] != 3:
        raise ValueError(f"{name}: verts must be [P,3], got {tuple(verts.shape)}")
    if tuple(origin.shape) != (B, 3):
        raise ValueError(f"{name}: origin must be [B,3] = {(B, 3)}, one camera centre per view of the lists, got {tuple(origin.shape)}")
    return _check_packed(name, "fragments.surface_packed is the torch path for anything else", frag, packed)


def surface_packed(frag, packed: PackedSlots, faces: th.Tensor, verts: th.Tensor, origin: th.Tensor) -> SurfaceRows:
    """The surface frame of every packed row -> SurfaceRows(hit, normal, reflect), each [N,3], N = packed.rows.  faces [F,3], verts
    [P,3], origin [B,3]: one camera centre per view of the lists (camera_origins(mv_mats)).  For a slot (b, k, y, x) that counts
    (0 <= row < N and a face id in [0, F)) with p0, p1, p2 the vertices of its face and (u, v) its barycentrics, in verts' dtype:
        h = (1 - u - v) p0 + u p1 + v p2                      == interpolate_packed(frag, packed, faces, verts)
        g = (p1 - p0) x (p2 - p0), a = |g|, m = g / a         m = 0 if a is not finite or a < 1e-20 (a degenerate face)
        w = h - origin[b], d = w / |w|                        d = 0 if |w| is not finite or |w| < 1e-8 (sh_rows' rule)
        s = m . d
        normal = m if s <= 0 else -m                          towards the camera: normal . d <= 0, whatever the face's winding
        reflect = d - 2 s m                                   unit length; d on a degenerate face, 0 where d = 0
    at row[b, k, y, x]; every other row is 0 (and so are the three rows of a slot whose face holds a vertex index outside [0, P)).
    The sign of the normal is a constant of every gradient.  Differentiable in verts (through the hit point and, unless the face is
    degenerate, through the normal), in frag.bary when the renderer's fragment_grads made it differentiable, and in origin.
    Plain torch, any device, any float dtype: the model surface_packed_fused is tested against."""
    rows = _check_surface("surface_packed", frag, packed, faces, verts, origin)
    F, P = faces.shape[0], verts.shape[0]
    B = frag.pix_to_face.shape[0]
    zero = th.zeros((), dtype=verts.dtype, device=verts.device)
    live = _counting(frag, packed, F)
    out = [verts.new_zeros(rows, 3) for _ in range(3)]
    if F == 0 or P == 0:   # no slot counts, or no face has its vertices
        return SurfaceRows(*out)
    vid = faces.long()[frag.pix_to_face.clamp(0, F - 1).long()[live]]                    # [n,3]
    inside = ((vid >= 0) & (vid < P)).all(1)
    p = verts[vid.clamp(0, P - 1)]                                                       # [n,3,3]
    bary = frag.bary.to(verts.dtype).permute(0, 1, 3, 4, 2)[live]                        # [n,2]
    u, v = bary[:, :1], bary[:, 1:]
    h = (1 - u - v) * p[:, 0] + u * p[:, 1] + v * p[:, 2]
    m, _ = _unit_or_zero(th.linalg.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), SURFACE_MIN_AREA)
    view = th.arange(B, device=live.device).view(B, 1, 1, 1).expand_as(live)[live]
    d, _ = _unit_or_zero(h - origin.to(verts.dtype)[view], SURFACE_MIN_LENGTH)
    s = (m * d).sum(1, keepdim=True)
    normal = th.where(s.detach() <= 0, m, -m)
    reflect = d - 2 * s * m
    at = (packed.row[live].long(),)
    return SurfaceRows(*(o.index_put(at, th.where(inside.unsqueeze(1), x, zero)) for o, x in zip(out, (h, normal, reflect))))


class _SurfacePackedFn(th.autograd.Function):
    """surface_packed_fused over _C.surface_packed / _C.surface_packed_backward.  Arguments: pix_to_face, bary, row, n_used, faces,
    verts, origin, rows.  Only those tensors are saved: the backward recomputes the frame."""

    @staticmethod
    def forward(ctx, face, bary, row, n_used, faces, verts, origin, rows):
        out = _fused_kernels("surface_packed").surface_packed(face, bary, row, n_used, faces, verts, origin, rows)
        ctx.save_for_backward(face, bary, row, n_used, faces, verts, origin)
        ctx.set_materialize_grads(False)  # an output the loss does not use arrives as None, and goes down as a null pointer: no zeros
        return tuple(out)

    @staticmethod
    def backward(ctx, grad_hit, grad_normal, grad_reflect):
        need = (ctx.needs_input_grad[5], ctx.needs_input_grad[1], ctx.needs_input_grad[6])  # (verts, bary, origin)
        ups = [None if g is None else g.contiguous() for g in (grad_hit, grad_normal, grad_reflect)]
        if all(g is None for g in ups) or not any(need):
            return (None,) * 8
        d_verts, d_bary, d_origin = _fused_kernels("surface_packed").surface_packed_backward(*ctx.saved_tensors, *ups, need)
        return None, d_bary, None, None, None, d_verts, d_origin, None


def surface_packed_fused(frag, packed: PackedSlots, faces: th.Tensor, verts: th.Tensor, origin: th.Tensor) -> SurfaceRows:
    """surface_packed(...) as one HIP kernel, and one for its backward (plus the one that zeroes dL_dverts and dL_dorigin): the same
    SurfaceRows(hit, normal, reflect), each [N,3]; hit equals interpolate_packed_fused(frag, packed, faces, verts) bit for bit.  The
    forward reads a face's three vertices once per counting slot and stores three 12-byte rows per lane; the backward merges the
    nine vertex-gradient floats of a wave's lanes of equal face, sums them per tile in an LDS table of f64 cells keyed by vertex
    and sums dL_dorigin per wave and per workgroup before at most three float atomics leave -- so dL_dverts and dL_dorigin depend
    on the order of summation in their last bits; the three outputs and dL_dbary do not.  A slot counts only if 0 <= row < N and
    its face id lies in [0, F): a `packed` made for another F or capacity stays in bounds; a face with a vertex index outside
    [0, P) gives three rows of zeros; rows [min(n_used, N), N) are exact zeros (the count is read on the device: no host wait,
    capturable).  Each gradient (verts, frag.bary, origin) is computed only when autograd asks for it, and an output the loss does
    not use sends no upstream down; dL_dbary is an exact 0 in slots that do not count.  N == 0 gives three empty [0,3] tensors
    without a launch.  K <= 32, origin [B,3] (ValueError).  HIP float32 / int32 tensors on one device only: anything else is a
    TypeError -- surface_packed is the torch path for it; nothing falls back silently."""
    name, torch_path = "surface_packed_fused", "fragments.surface_packed is the torch path for anything else"
    _fused_kernels("surface_packed")
    rows = _check_surface(name, frag, packed, faces, verts, origin)
    ints = [("faces", faces), ("packed.row", packed.row), ("packed.n_used", packed.n_used)]
    _check_tensors(name, torch_path, frag.pix_to_face, ints, [("frag.bary", frag.bary), ("verts", verts), ("origin", origin)])
    if rows == 0:
        return SurfaceRows(*(verts.new_zeros((0, 3)) for _ in range(3)))
    return SurfaceRows(*_SurfacePackedFn.apply(frag.pix_to_face, frag.bary, packed.row, packed.n_used, faces.to(th.int32), verts, origin, rows))
