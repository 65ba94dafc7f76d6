"""Independent float64 reference for the tet renderer's camera gradients (TetRenderer(camera_grads=True)).

Extends tests/tet_grad_ref.py's brute-force model, and keeps its pixel selection and each kept pixel's face order.  The
rays are no longer the oracle's: every kept pixel's ray is rebuilt from float64 leaf matrices, as pixel_ray<true> builds
it.  The origin is inv_mv's translation column.  The direction is normalize(inv_mv (inv_proj (ndc, -1, 1)).xyz - origin),
with no w divide and the length clamped to 1e-4 (no +1e-7 as on the tri side); the inverses come from th.inverse.  The
ndc a pixel's ray goes through is a constant: the pixel centre, or with a ray_random_seed the oracle's jittered sample,
recovered by projecting its ray_o + ray_d back through proj . mv in float64.  With mv_mats and proj_mats among the
autograd leaves, torch.autograd gives their gradients through the rays and through each hit point's ndc depth; no chain
rule is written by hand.
"""
from __future__ import annotations

from typing import Dict

import numpy as np
import torch as th

import tet_grad_ref
from tet_grad_ref import TetGradRef

KEYS = tet_grad_ref.KEYS + ("mv_mats", "proj_mats")


class TetCameraGradRef(TetGradRef):
    """TetGradRef whose rays depend on the (row-major, Module) matrices.  seed: the scene's ray_random_seed."""

    def __init__(self, d: Dict[str, th.Tensor], H: int, W: int, st, seed: int = 0, chunk: int = 1024):
        super().__init__(d, H, W, st, chunk)
        r = self.pix % (H * W)
        px, py = (r % W).to(th.float64), (r // W).to(th.float64)
        if seed > 0:
            X = th.cat([self.ro + self.rd, th.ones(self.ro.shape[0], 1, dtype=th.float64)], 1)
            M = d["proj_mats"].to(th.float64)[self.view] @ d["mv_mats"].to(th.float64)[self.view]
            clip = (M @ X[:, :, None])[:, :, 0]
            self.ndc = clip[:, :2] / clip[:, 3:]
        else:
            self.ndc = th.stack([((px + 0.5) * 2 + 1) / W - 1, ((py + 0.5) * 2 + 1) / H - 1], 1)

    def rays(self, mv: th.Tensor, proj: th.Tensor):
        """(o, d) [N,3] of the kept pixels from row-major [B,4,4] matrices (differentiable)."""
        im, ip = th.inverse(mv)[self.view], th.inverse(proj)[self.view]
        one = th.ones(self.ndc.shape[0], 1, dtype=mv.dtype)
        ndc = th.cat([self.ndc.to(mv.dtype), -one, one], 1)
        pv = (ip @ ndc[:, :, None])[:, :, 0]
        pw = (im[:, :3, :3] @ pv[:, :3, None])[:, :, 0] + im[:, :3, 3]
        o = im[:, :3, 3]
        w = pw - o
        return o, w / th.sqrt((w * w).sum(-1, keepdim=True)).clamp(min=1e-4)

    def render(self, inputs: Dict[str, th.Tensor]):
        """TetGradRef.render with the rays and the depth's matrices taken from inputs["mv_mats"], inputs["proj_mats"]."""
        kept = self.d, self.ro, self.rd
        self.ro, self.rd = self.rays(inputs["mv_mats"], inputs["proj_mats"])
        self.d = dict(self.d, mv_mats=inputs["mv_mats"], proj_mats=inputs["proj_mats"])
        try:
            return super().render(inputs)
        finally:
            self.d, self.ro, self.rd = kept

    def leaves(self) -> Dict[str, th.Tensor]:
        return {k: self.d[k].to(th.float64).clone() for k in KEYS}

    def loss(self, inputs: Dict[str, th.Tensor], gc: th.Tensor, gd: th.Tensor):
        """(sum(gc * color) + sum(gd * depth) over the kept pixels, color [N,3], depth [N])."""
        color, depth = self.render(inputs)
        HW = self.H * self.W
        b, r = self.view, self.pix % HW
        gcf = gc.to(th.float64).reshape(self.B, 3, HW)[b, :, r]
        gdf = gd.to(th.float64).reshape(self.B, HW)[b, r]
        return (color * gcf).sum() + (depth * gdf).sum(), color, depth

    def grads(self, gc: th.Tensor, gd: th.Tensor):
        """Gradients of the loss in float64 for every key of KEYS (the matrices row-major, as the Module takes them),
        and the forward (color [N,3], depth [N])."""
        leaves = {k: v.requires_grad_(True) for k, v in self.leaves().items()}
        L, color, depth = self.loss(leaves, gc, gd)
        L.backward()
        return {k: v.grad.numpy() for k, v in leaves.items()}, color.detach(), depth.detach()

    def finite_differences(self, key: str, gc: th.Tensor, gd: th.Tensor, h: float = 1e-6) -> np.ndarray:
        """Central differences of the loss in every entry of inputs[key] (the march order is fixed: well defined)."""
        base = self.leaves()
        out = np.zeros(tuple(base[key].shape))
        with th.no_grad():
            for idx in np.ndindex(*out.shape):
                vals = []
                for s in (1.0, -1.0):
                    x = dict(base)
                    x[key] = base[key].clone()
                    x[key][idx] += s * h
                    vals.append(float(self.loss(x, gc, gd)[0]))
                out[idx] = (vals[0] - vals[1]) / (2 * h)
        return out
