"""Float64 model of the tri renderer's fragment gradients (TriRenderer(..., return_fragments=K, fragment_grads=True);
`fragment_grads=(pix_to_face, grad_bary)` of _C.render_tris_backward; DMR_FLAG_TRI_FRAGMENT_GRADS).

Built from tests/tri_grad_ref.py's pieces (pixel_rays, _uv, _clamp, _clamp_border_dist): given (view, y, x, face) pairs and an
upstream g [N,2], autograd of sum(g . (u_c, v_c)) gives the gradients of verts, mv_mats and proj_mats (the row-major Module
matrices) with no chain rule written by hand.  Plain torch on the CPU; imported by tests/test_fragment_grads_{cpu,gpu}.py.
"""
from __future__ import annotations

from typing import Dict

import numpy as np
import torch as th

from tri_grad_ref import _clamp, _clamp_border_dist, _uv, pixel_rays

BORDER_EPS = 1e-4  # pairs within BORDER_EPS * max(1, |u|, |v|) of a border between two clamp regions get no upstream


def regions(u: th.Tensor, v: th.Tensor) -> th.Tensor:
    """The clamp region 0..6 of (u, v): clamp_bary_uv's `code`, the conditions of tri_grad_ref._clamp in its order."""
    conds = [(u >= 0) & (v >= 0) & (u + v <= 1), (u <= 0) & (v <= 0), ((u >= 1) & (v <= 0)) | ((v >= 0) & (v <= u - 1)),
             ((u <= 0) & (v >= 1)) | ((u >= 0) & (v >= u + 1)), (u <= 0) & (v <= 1) & (v >= 0), (u <= 1) & (u >= 0) & (v <= 0)]
    code = th.full(u.shape, 6, dtype=th.int64)
    for c in reversed(range(6)):
        code = th.where(conds[c], th.full_like(code, c), code)
    return code


class Pairs:
    """(view, y, x, face) pairs of a scene dict d (row-major matrices) and their float64 forward: u, v (unclamped), region,
    distance to the nearest clamp border."""

    def __init__(self, d: Dict[str, th.Tensor], H: int, W: int, view, py, px, face):
        self.d, self.H, self.W = d, H, W
        self.view, self.py, self.px, self.face = (th.as_tensor(t).long() for t in (view, py, px, face))
        with th.no_grad():
            self.u, self.v = self._uv({k: d[k].to(th.float64) for k in ("verts", "mv_mats", "proj_mats")})
        self.region = regions(self.u, self.v)
        self.border = _clamp_border_dist(self.u, self.v)

    def _uv(self, x):
        faces = self.d["faces"].long()
        o, dr = pixel_rays(x["mv_mats"], x["proj_mats"], self.view, self.px, self.py, self.H, self.W)
        i = faces[self.face]
        return _uv(o, dr, x["verts"][i[:, 0]], x["verts"][i[:, 1]], x["verts"][i[:, 2]])

    def near_border(self) -> th.Tensor:
        scale = th.maximum(th.ones_like(self.u), th.maximum(self.u.abs(), self.v.abs()))
        return self.border < BORDER_EPS * scale

    def clamped(self):
        return _clamp(self.u, self.v)

    def grads(self, g: th.Tensor) -> Dict[str, np.ndarray]:
        """d sum(g . (u_c, v_c)) / d(verts, mv_mats, proj_mats); g [N,2]."""
        leaves = {k: self.d[k].to(th.float64).clone().requires_grad_(True) for k in ("verts", "mv_mats", "proj_mats")}
        uc, vc = _clamp(*self._uv(leaves))
        g = g.to(th.float64)
        (uc * g[:, 0] + vc * g[:, 1]).sum().backward()
        return {k: t.grad.numpy() for k, t in leaves.items()}


def pairs_of_lists(d, H, W, face: th.Tensor, pixels=None) -> "tuple[Pairs, tuple]":
    """The pairs of a face tensor [B,K,H,W] with ids inside [0, F) -- on the pixels of the mask `pixels` [B,H,W] only, if
    given -> (Pairs, (b, k, y, x) of each)."""
    F = d["faces"].shape[0]
    face = th.as_tensor(face).long()
    sel = (face >= 0) & (face < F)
    if pixels is not None:
        sel = sel & (th.as_tensor(pixels) > 0)[:, None]
    b, k, y, x = th.nonzero(sel, as_tuple=True)
    return Pairs(d, H, W, b, y, x, face[b, k, y, x]), (b, k, y, x)


SYNTH = dict(L=3, n=9, B=2, H=40, W=56, K=3, scene_seed=7, opacity=(0.1, 0.5), seed=1)


def synthetic(far: float = float("inf")):
    """Test 1's pairs: on a small ragged frame every slot of every pixel gets a face drawn uniformly from [-1, F), so most rays
    miss their face and every clamp region is reached; N(0, 1) upstream, zero for pairs near a clamp border (BORDER_EPS) and,
    with `far`, for pairs whose max(|u|, |v|) exceeds it.
    -> (scene dict, B, H, W, K, face int32 [B,K,H,W], grad_bary float32 [B,K,2,H,W], Pairs, their upstream [N,2], dropped
    mask [N])."""
    from dmesh_renderer_amd import scenes
    s = SYNTH
    B, H, W, K = s["B"], s["H"], s["W"], s["K"]
    d = scenes.layered_sheets(s["L"], s["n"], B, H, W, seed=s["scene_seed"], opacity=s["opacity"])
    F = d["faces"].shape[0]
    gen = th.Generator().manual_seed(s["seed"])
    face = th.randint(-1, F, (B, K, H, W), generator=gen, dtype=th.int64)
    gb = th.randn(B, K, 2, H, W, generator=gen)
    pairs, (b, k, y, x) = pairs_of_lists(d, H, W, face)
    dropped = pairs.near_border()
    keep = ~dropped & (th.maximum(pairs.u.abs(), pairs.v.abs()) <= far)
    mask = th.zeros(B, K, H, W)
    mask[b, k, y, x] = keep.to(mask.dtype)
    gb = gb * mask[:, :, None]
    return d, B, H, W, K, face.int(), gb.contiguous(), pairs, gb[b, k, :, y, x].clone(), dropped
