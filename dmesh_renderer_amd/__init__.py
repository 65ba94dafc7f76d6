"""dmesh_renderer_amd -- MI355X-native drop-in for the hot path of SonSang/dmesh_renderer.

Public surface = the reference package's (dmesh_renderer/__init__.py):
    TriRenderSettings, render_tri, TriRenderer      (:13-16, :18-43, :172-225)
    TetRenderSettings, render_tet, TetRenderer      (:237-241, :243-275, :426-488)
with identical argument order, dtypes, shapes, outputs and gradient routing.  The compute
lives in libdmesh_renderer_hip.so (hand-written gfx950 kernels) behind `_C`.

Conventions kept from the reference: the Modules receive ROW-major [B,4,4] matrices and
pass transposed views down (:219-220, :476-477); the autograd Functions invert those
(:62-63, :298-299); the tri Module only casts `faces`, the tet Module casts everything (Q23).
"""
from __future__ import annotations

from typing import NamedTuple, Tuple

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

__all__ = ["TriRenderSettings", "render_tri", "TriRenderer", "TetRenderSettings", "render_tet", "TetRenderer"]


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


def _tri_grad_keywords(exact_grads: bool, camera_grads: bool) -> dict:
    """The keywords of _C.render_tris_backward for the tri gradient options: none by default (the reference's call)."""
    if camera_grads:
        return {"camera_grads": True}
    return {"exact_grads": True} if exact_grads else {}


class _TriFn(th.autograd.Function):
    """Inputs: verts, faces, verts_color, faces_opacity, mv^T, proj^T, verts_depth, faces_intense,
    settings, rows[, exact_grads, camera_grads].  Gradients flow to verts, verts_color, faces_opacity, verts_depth,
    faces_intense; with camera_grads also to mv^T and proj^T (see TriRenderer)."""

    @staticmethod
    def forward(ctx, verts, faces, verts_color, faces_opacity, mv_mats, proj_mats, verts_depth, faces_intense,
                settings: TriRenderSettings, rows, exact_grads=False, camera_grads=False):
        cams = _with_inverses(mv_mats, proj_mats)
        geom = (verts, faces, verts_color, faces_opacity)
        try:
            out = _C.render_tris(settings.bg, *geom, *cams, verts_depth, faces_intense,
                                 settings.image_height, settings.image_width, rows=rows)
        except Exception as ex:
            print("\nAn error occured in forward.")
            print(ex)
            raise
        num_rendered, color, depth = out[0], out[1], out[2]
        ctx.settings, ctx.rows, ctx.num_rendered = settings, rows, num_rendered
        ctx.exact_grads, ctx.camera_grads = exact_grads or camera_grads, camera_grads
        ctx.save_for_backward(*geom, *cams, verts_depth, faces_intense, *out[3:7])
        return color, depth

    @staticmethod
    def backward(ctx, grad_color, grad_depth):
        saved = ctx.saved_tensors
        inputs, scratch = saved[:10], saved[10:14]
        # the matrices' gradients only when asked for: otherwise the exact variant, which skips the per-pixel ray sums
        camera = ctx.camera_grads and (ctx.needs_input_grad[4] or ctx.needs_input_grad[5])
        try:
            g = _C.render_tris_backward(ctx.settings.bg, *inputs, grad_color, grad_depth, ctx.num_rendered,
                                        *scratch, rows=ctx.rows, **_tri_grad_keywords(ctx.exact_grads, camera))
        except Exception:
            print("\nAn error occured in backward.\n")
            raise
        g_verts, g_vcolor, g_fopacity, g_vdepth, g_fintense = g[:5]
        g_mv = g_proj = None
        if camera:  # dL/d(inverse) -> dL/d(matrix); saved[6:8] are the inverses the forward used
            g_mv = _through_inverse(saved[6], g[5]) if ctx.needs_input_grad[4] else None
            g_proj = _through_inverse(saved[7], g[6]) if ctx.needs_input_grad[5] else None
        return g_verts, None, g_vcolor, g_fopacity, g_mv, g_proj, g_vdepth, g_fintense, None, None, None, None


class _TetFn(th.autograd.Function):
    """Gradients flow to verts_color and faces_opacity only (reference :407-422); with full_grads also to verts and
    faces_intense (beyond the reference)."""

    @staticmethod
    def forward(ctx, verts, faces, verts_color, faces_opacity, mv_mats, proj_mats, verts_depth, faces_intense,
                tets, face_tets, tet_faces, settings: TetRenderSettings, rows, full_grads=False):
        cams = _with_inverses(mv_mats, proj_mats)
        geom = (verts, faces, verts_color, faces_opacity)
        topo = (tets, face_tets, tet_faces)
        try:
            out = _C.render_tets(settings.bg, *geom, *cams, verts_depth, faces_intense, *topo,
                                 settings.image_height, settings.image_width, settings.ray_random_seed, rows=rows)
        except Exception:
            print("\nAn error occured in forward.")
            raise
        color, depth, active = out[0], out[1], out[2] > 0.5  # bool mask, reference :333
        ctx.settings, ctx.rows, ctx.full_grads = settings, rows, full_grads
        ctx.save_for_backward(*geom, *cams, verts_depth, faces_intense, *topo, *out[3:7])
        ctx.mark_non_differentiable(active)
        return color, depth, active

    @staticmethod
    def backward(ctx, grad_color, grad_depth, _grad_active):
        saved = ctx.saved_tensors
        inputs, scratch = saved[:13], saved[13:17]
        g_verts = g_fintense = None
        try:
            if ctx.full_grads:  # (the keyword is only passed when set: the default call is the reference's)
                g_verts, g_vcolor, g_fopacity, g_fintense = _C.render_tets_backward(
                    ctx.settings.bg, *inputs, grad_color, grad_depth, *scratch, rows=ctx.rows, full_grads=True)
            else:
                g_vcolor, g_fopacity = _C.render_tets_backward(ctx.settings.bg, *inputs, grad_color, grad_depth,
                                                               *scratch, rows=ctx.rows)
        except Exception:
            print("\nAn error occured in backward.\n")
            raise
        return (g_verts, None, g_vcolor, g_fopacity, None, None, None, g_fintense) + (None,) * 6


def render_tri(verts, faces, verts_color, faces_opacity, mv_mats, proj_mats, verts_depth, faces_intense,
               render_settings: TriRenderSettings, rows=(0, 0), exact_grads=False, camera_grads=False):
    """Functional form (reference :18-43).  mv_mats / proj_mats are the TRANSPOSED matrices.  exact_grads,
    camera_grads: see TriRenderer."""
    opts = (bool(exact_grads), bool(camera_grads)) if exact_grads or camera_grads else ()
    return _TriFn.apply(verts, faces, verts_color, faces_opacity, mv_mats, proj_mats, verts_depth,
                        faces_intense, render_settings, tuple(rows), *opts)


def render_tet(verts, faces, verts_color, faces_opacity, mv_mats, proj_mats, verts_depth, faces_intense,
               tets, face_tets, tet_faces, render_settings: TetRenderSettings, rows=(0, 0), full_grads=False):
    """Functional form (reference :243-275).  mv_mats / proj_mats are the TRANSPOSED matrices.  full_grads: see
    TetRenderer."""
    return _TetFn.apply(verts, faces, verts_color, faces_opacity, mv_mats, proj_mats, verts_depth,
                        faces_intense, tets, face_tets, tet_faces, render_settings, tuple(rows), bool(full_grads))


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

    forward(verts [P,3], faces [F,3], verts_color [P,3], faces_opacity [F],
            mv_mats [B,4,4], proj_mats [B,4,4], verts_depth [B,P], faces_intense [B,F])
        -> color [B,3,H,W], depth [B,1,H,W]
    """

    def __init__(self, render_settings: TriRenderSettings, exact_grads: bool = False, camera_grads: bool = False):
        super().__init__()
        self.render_settings = render_settings
        self.exact_grads = bool(exact_grads)
        self.camera_grads = bool(camera_grads)

    def forward(self, verts, faces, verts_color, faces_opacity, mv_mats, proj_mats, verts_depth, faces_intense):
        return render_tri(verts, faces.to(dtype=th.int32), verts_color, faces_opacity,
                          mv_mats.transpose(1, 2), proj_mats.transpose(1, 2), verts_depth, faces_intense,
                          self.render_settings, exact_grads=self.exact_grads, camera_grads=self.camera_grads)


class TetRenderer(th.nn.Module):
    """Renderer for the faces of a compact set of tetrahedra: the ray is marched tet to tet, so
    faces are composited in exact depth order; gradients reach verts_color and faces_opacity only
    (reference README.md:4).

    full_grads=True (beyond the reference, which has no such gradients): gradients also reach verts and
    faces_intense.  On the forward's march each composited face enters through the ray's hit (t, u, v) on it: u, v
    set its interpolated colour, t the hit point and so its ndc depth; the march itself (which faces, in which order)
    and the opacities are constants of the gradient.  verts_depth (not read by this renderer) and the matrices get
    none.  Costs a slower backward; the forward is the same.

    forward(verts, faces, verts_color, faces_opacity, mv_mats, proj_mats, verts_depth, faces_intense,
            tets [T,4], face_tets [F,2] (-1 = none), tet_faces [T,4])
        -> color [B,3,H,W], depth [B,1,H,W], active bool [B,H,W]
    """

    def __init__(self, render_settings: TetRenderSettings, full_grads: bool = False):
        super().__init__()
        self.render_settings = render_settings
        self.full_grads = bool(full_grads)

    def forward(self, verts, faces, verts_color, faces_opacity, mv_mats, proj_mats, verts_depth, faces_intense,
                tets, face_tets, tet_faces):
        f32, i32 = dict(dtype=th.float32), dict(dtype=th.int32)
        return render_tet(verts.to(**f32), faces.to(**i32), verts_color.to(**f32), faces_opacity.to(**f32),
                          mv_mats.to(**f32).transpose(1, 2), proj_mats.to(**f32).transpose(1, 2),
                          verts_depth.to(**f32), faces_intense.to(**f32),
                          tets.to(**i32), face_tets.to(**i32), tet_faces.to(**i32), self.render_settings,
                          full_grads=self.full_grads)
