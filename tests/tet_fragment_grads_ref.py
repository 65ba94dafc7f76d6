"""Float64 model of the tet renderer's fragment gradients (TetRenderer(..., return_fragments=K, fragment_grads=True);
`fragment_grads=(pix_to_face, grad_bary)` of _C.render_tets_backward; DMR_FLAG_TET_FRAGMENT_GRADS).

Given (view, y, x, face) pairs and an upstream g [N,2], autograd of sum(g . (u, v)) gives the gradients of verts, mv_mats and
proj_mats (the row-major Module matrices) with no chain rule written by hand.  The rays are built from the leaf matrices
exactly as tests/tet_camera_grad_ref.py's TetCameraGradRef.rays builds them (origin inv_mv's translation column, direction
w / max(|w|, 1e-4), no w divide), through the pixel centre or through the jittered ndc samples passed in; (u, v, den) are
tests/tet_grad_ref.py's _hits: the unclamped Moeller-Trumbore (u, v).  Plain torch on the CPU; imported by
tests/test_tet_fragment_grads_{cpu,gpu}.py.

Selection rule: a pair whose ray grazes its face -- |den| / (|E1 x E2| |d|), the cosine between the ray and the face's normal,
below GRAZING_EPS = 1e-2 -- gets a zero upstream, the exact den == 0 pairs of the axis-aligned Kuhn faces seen edge-on among
them.  d(u, v) grows like 1 / den^2 there: a handful of such pairs would own the whole comparison (max |ref| 2.5e16 on the
synthetic set without the rule).  The kernel skips pairs with a zero upstream, so their terms enter neither side.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch as th

from tet_grad_ref import _hits

GRAZING_EPS = 1e-2
LEAVES = ("verts", "mv_mats", "proj_mats")


def rays(mv: th.Tensor, proj: th.Tensor, view: th.Tensor, ndc: th.Tensor):
    """(o, d) [N,3] of rays through `ndc` [N,2] of the views `view` from row-major [B,4,4] matrices (differentiable):
    TetCameraGradRef.rays."""
    im, ip = th.inverse(mv)[view], th.inverse(proj)[view]
    one = th.ones(ndc.shape[0], 1, dtype=mv.dtype)
    q = th.cat([ndc.to(mv.dtype), -one, one], 1)
    pv = (ip @ q[:, :, None])[:, :, 0]
    pw = (im[:, :3, :3] @ pv[:, :3, None])[:, :, 0] + im[:, :3, 3]
    o = im[:, :3, 3]
    w = pw - o
    return o, w / th.sqrt((w * w).sum(-1, keepdim=True)).clamp(min=1e-4)


def pixel_centres(px: th.Tensor, py: th.Tensor, H: int, W: int) -> th.Tensor:
    """The ndc of the pixel centres (pix2ndc of px + 0.5, py + 0.5), float64 [N,2]."""
    px, py = px.to(th.float64), py.to(th.float64)
    return th.stack([((px + 0.5) * 2 + 1) / W - 1, ((py + 0.5) * 2 + 1) / H - 1], 1)


class TetPairs:
    """(view, y, x, face) pairs of a scene dict d (row-major matrices) and their float64 forward: the unclamped u, v, den and
    the grazing measure.  ndc [N,2]: the samples the rays go through (a jittered scene's); None: the pixel centres."""

    def __init__(self, d: Dict[str, th.Tensor], H: int, W: int, view, py, px, face, ndc: Optional[th.Tensor] = None):
        self.d, self.H, self.W = d, H, W
        self.view, self.py, self.px, self.face = (th.as_tensor(t).long() for t in (view, py, px, face))
        self.ndc = pixel_centres(self.px, self.py, H, W) if ndc is None else th.as_tensor(ndc).to(th.float64)
        with th.no_grad():
            x = {k: d[k].to(th.float64) for k in LEAVES}
            self.u, self.v, self.den, self.grazing = self._uv(x, measure=True)

    def _uv(self, x, measure=False, on=slice(None)):
        i = self.d["faces"].long()[self.face[on]]
        o, dr = rays(x["mv_mats"], x["proj_mats"], self.view[on], self.ndc[on])
        p0, p1, p2 = x["verts"][i[:, 0]], x["verts"][i[:, 1]], x["verts"][i[:, 2]]
        _, u, v, den = _hits(o, dr, p0, p1, p2)
        if not measure:
            return u, v
        n = th.cross(p1 - p0, p2 - p0, dim=-1)
        return u, v, den, den.abs() / (n.norm(dim=-1) * dr.norm(dim=-1))

    def grazes(self) -> th.Tensor:
        """The pairs the selection rule drops (den == 0 among them: their measure is 0)."""
        return ~(self.grazing >= GRAZING_EPS)

    def loss(self, x: Dict[str, th.Tensor], g: th.Tensor) -> th.Tensor:
        """sum(g . (u, v)) over the pairs with a non-zero upstream, from leaves x (LEAVES) of any float dtype."""
        on = (g != 0).any(1)  # (a pair without upstream is not evaluated: 0 * inf is never formed, forward or backward)
        u, v = self._uv(x, on=on)
        g = g[on].to(u.dtype)
        return (u * g[:, 0] + v * g[:, 1]).sum()

    def hit_grads(self, up: th.Tensor) -> Dict[str, np.ndarray]:
        """d sum(up . hit) / d(verts, mv_mats, proj_mats) for hit = (1 - u - v) p0 + u p1 + v p2, up [N,3]: the FULL derivative
        of the hit points -- the direct term through the three vertex rows plus the term through the movement of (u, v)."""
        x = {k: t.requires_grad_(True) for k, t in self.leaves().items()}
        on = (up != 0).any(1)
        u, v = self._uv(x, on=on)
        i = self.d["faces"].long()[self.face[on]]
        p0, p1, p2 = x["verts"][i[:, 0]], x["verts"][i[:, 1]], x["verts"][i[:, 2]]
        hit = (1 - u - v)[:, None] * p0 + u[:, None] * p1 + v[:, None] * p2
        (hit * up[on].to(th.float64)).sum().backward()
        return {k: t.grad.numpy() for k, t in x.items()}

    def leaves(self, dtype=th.float64) -> Dict[str, th.Tensor]:
        return {k: self.d[k].to(dtype).clone() for k in LEAVES}

    def grads(self, g: th.Tensor, dtype=th.float64) -> Dict[str, np.ndarray]:
        """d sum(g . (u, v)) / d(verts, mv_mats, proj_mats); g [N,2].  dtype float32: the same formula through float32
        autograd, the proxy for what single precision can do on these inputs."""
        x = {k: t.requires_grad_(True) for k, t in self.leaves(dtype).items()}
        keep = self.ndc
        self.ndc = self.ndc.to(dtype)
        try:
            self.loss(x, g).backward()
        finally:
            self.ndc = keep
        return {k: t.grad.double().numpy() for k, t in x.items()}


def pairs_of_lists(d, H, W, face: th.Tensor, pixels=None, ndc=None) -> "tuple[TetPairs, tuple]":
    """The pairs of a face tensor [B,K,H,W] with ids inside [0, F) -- on the pixels of the mask `pixels` [B,H,W] only, if
    given -> (TetPairs, (b, k, y, x) of each).  ndc [B,H,W,2]: every pixel's sample (None: the pixel centres)."""
    F = d["faces"].shape[0]
    face = th.as_tensor(face).long()
    sel = (face >= 0) & (face < F)
    if pixels is not None:
        sel = sel & (th.as_tensor(pixels) > 0)[:, None]
    b, k, y, x = th.nonzero(sel, as_tuple=True)
    return TetPairs(d, H, W, b, y, x, face[b, k, y, x], None if ndc is None else th.as_tensor(ndc)[b, y, x]), (b, k, y, x)


def masked_upstream(shape, pairs: TetPairs, where, gen: th.Generator):
    """N(0, 1) upstream [B,K,2,H,W] on the pairs `where` = (b, k, y, x) that do not graze, zero elsewhere
    -> (grad_bary float32, its rows [N,2] of the pairs, the dropped mask [N])."""
    b, k, y, x = where
    B, K, _, H, W = shape
    gb = th.randn(*shape, generator=gen)
    dropped = pairs.grazes()
    mask = th.zeros(B, K, H, W)
    mask[b, k, y, x] = (~dropped).to(mask.dtype)
    gb = (gb * mask[:, :, None]).contiguous()
    return gb, gb[b, k, :, y, x].clone(), dropped


SYNTH = dict(m=4, B=2, H=40, W=56, K=3, scene_seed=0, opacity=(0.05, 0.5), seed=1)


def synthetic():
    """Test 1's pairs: on a small frame, ragged in both directions, every slot of every pixel gets a face drawn uniformly
    from [-1, F), so the pairs are not the march's: most rays miss their face and (u, v) is far outside the triangle; N(0, 1)
    upstream, zero for the pairs that graze.
    -> (scene dict, B, H, W, K, face int32 [B,K,H,W], grad_bary float32 [B,K,2,H,W], TetPairs, their upstream [N,2], dropped
    mask [N])."""
    from dmesh_renderer_amd import scenes
    s = SYNTH
    B, H, W, K = s["B"], s["H"], s["W"], s["K"]
    d = scenes.kuhn_tets(s["m"], B, H, W, seed=s["scene_seed"], opacity=s["opacity"])
    F = d["faces"].shape[0]
    gen = th.Generator().manual_seed(s["seed"])
    face = th.randint(-1, F, (B, K, H, W), generator=gen, dtype=th.int64)
    pairs, where = pairs_of_lists(d, H, W, face)
    gb, g, dropped = masked_upstream((B, K, 2, H, W), pairs, where, gen)
    return d, B, H, W, K, face.int(), gb, pairs, g, dropped


def finite_difference(pairs: TetPairs, g: th.Tensor, key: str, idx, h: float = 1e-6) -> float:
    """Central difference of the float64 loss in entry `idx` of leaf `key` (the pairs are fixed: well defined)."""
    vals = []
    with th.no_grad():
        for s in (1.0, -1.0):
            x = pairs.leaves()
            x[key][idx] += s * h
            vals.append(float(pairs.loss(x, g)))
    return (vals[0] - vals[1]) / (2 * h)
