"""Independent float64 reference for the tri renderer's exact and camera gradients (TriRenderer(exact_grads=True,
camera_grads=True)).

The CPU oracle supplies what the model does not decide: each tile's depth-sorted face list (`values` / `ranges`), the
projected vertices (`image`) and, per pixel, n_contrib.  Everything else is recomputed in float64 with torch ops, so
that autograd gives the gradients with no chain rule written by hand:
  - the pixel rays from the row-major Module matrices, as pixel_ray does (o = inv_mv's translation column,
    d = normalize(inv_mv (inv_proj (ndc, -1, 1)).xyz - o) with +1e-7 in the length), the inverses through th.inverse;
  - coverage: float64 point-in-triangle of the pixel centre on the oracle's `image` coordinates;
  - per pair the Moeller-Trumbore (u, v), the clamp of clamp_bary_uv, the interpolated colour and depth;
  - compositing like the oracle's tri_render_tile: blend, then stop when T < T_EPS.
Dropped (their upstream gradients are zeroed by `mask`, for the model and for the renderer under test alike): pixels
whose centre lies within EDGE_EPS pixels of an edge of a listed face (the fixed-point coverage test may decide those
either way), pixels whose blended pairs' (u, v) lie within CLAMP_EPS of a border of the clamp regions, and pixels
whose walk does not end at the oracle's n_contrib.
"""
from __future__ import annotations

from typing import Dict

import numpy as np
import torch as th

T_EPS = 1e-4  # auxiliary.h:8
EDGE_EPS = 0.1  # pixels: the coverage test snaps the vertices to 1/16 pixel (truncating)
CLAMP_EPS = 1e-4
KEYS = ("verts", "verts_color", "faces_opacity", "verts_depth", "faces_intense", "mv_mats", "proj_mats")


def pixel_rays(mv: th.Tensor, proj: th.Tensor, view: th.Tensor, px: th.Tensor, py: th.Tensor, H: int, W: int):
    """(o, d) [N,3] of pixels (view, px, py) from row-major [B,4,4] Module matrices (any float dtype, differentiable)."""
    im, ip = th.inverse(mv)[view], th.inverse(proj)[view]
    one = th.ones_like(px, dtype=mv.dtype)
    ndc = th.stack([((px.to(mv.dtype) + 0.5) * 2 + 1) / W - 1, ((py.to(mv.dtype) + 0.5) * 2 + 1) / H - 1, -one, one], -1)
    pv = (ip @ ndc[:, :, None])[:, :, 0]
    pw = (im[:, :3, :3] @ pv[:, :3, None])[:, :, 0] + im[:, :3, 3]
    o = im[:, :3, 3]
    w = pw - o
    d = w / (th.sqrt((w * w).sum(-1, keepdim=True)) + 1e-7)
    return o, d


def _uv(o, d, p0, p1, p2):
    T, E1, E2 = o - p0, p1 - p0, p2 - p0
    P = th.cross(d, E2, dim=-1)
    den = (P * E1).sum(-1)
    Q = th.cross(T, E1, dim=-1)
    return (P * T).sum(-1) / den, (Q * d).sum(-1) / den


def _clamp(u, v):
    """clamp_bary_uv (auxiliary.h:335-372) with torch.where: its piecewise Jacobian comes with it."""
    z, one = th.zeros_like(u), th.ones_like(u)
    c0 = (u >= 0) & (v >= 0) & (u + v <= 1)
    c1 = (u <= 0) & (v <= 0)
    c2 = ((u >= 1) & (v <= 0)) | ((v >= 0) & (v <= u - 1))
    c3 = ((u <= 0) & (v >= 1)) | ((u >= 0) & (v >= u + 1))
    c4 = (u <= 0) & (v <= 1) & (v >= 0)
    c5 = (u <= 1) & (u >= 0) & (v <= 0)
    uc = th.where(c0, u, th.where(c1, z, th.where(c2, one, th.where(c3, z, th.where(c4, z, th.where(c5, u, (1 + u - v) * 0.5))))))
    vc = th.where(c0, v, th.where(c1, z, th.where(c2, z, th.where(c3, one, th.where(c4, v, th.where(c5, z, (1 - u + v) * 0.5))))))
    return uc, vc


def _clamp_border_dist(u, v):
    """Distance of (u, v) to the nearest border between two clamp regions."""
    lines = th.stack([u, v, u + v - 1, u - 1, v - 1, (v - u + 1) / np.sqrt(2), (v - u - 1) / np.sqrt(2)], -1)
    return lines.abs().min(-1).values


class TriGradRef:
    """Selection and float64 forward / gradients of one scene.  d: a scenes.* dict (row-major matrices); st: the
    oracle's tri_forward state of the same scene."""

    def __init__(self, d: Dict[str, th.Tensor], H: int, W: int, st):
        self.d, self.H, self.W = d, H, W
        B = d["mv_mats"].shape[0]
        P = d["verts"].shape[0]
        self.B = B
        gx, gy = (W + 15) // 16, (H + 15) // 16
        ranges = st.get("ranges").astype(np.int64).reshape(-1, 2)
        values = st.get("values").astype(np.int64)
        image = th.from_numpy(st.get("image").reshape(B, P, 2).astype(np.float64))
        n_contrib = st.get("n_contrib").astype(np.int64).reshape(B, H, W)
        faces = d["faces"].long()
        f64 = th.float64
        with th.no_grad():
            self.ray_o, self.ray_d = self._all_rays(d["mv_mats"].to(f64), d["proj_mats"].to(f64))
        keep = np.zeros((B, H, W), bool)
        lists = {}
        K = 1
        for b in range(B):
            for ty in range(gy):
                for tx in range(gx):
                    r0, r1 = ranges[b * gx * gy + ty * gx + tx]
                    ys, xs = np.meshgrid(np.arange(ty * 16, min(H, ty * 16 + 16)), np.arange(tx * 16, min(W, tx * 16 + 16)), indexing="ij")
                    ys, xs = ys.reshape(-1), xs.reshape(-1)
                    if r1 <= r0:
                        keep[b, ys, xs] = n_contrib[b, ys, xs] == 0
                        continue
                    fl = th.from_numpy(values[r0:r1])
                    tri = image[b][faces[fl]]                                         # [n, 3, 2]
                    c = th.stack([th.from_numpy(xs + 0.5), th.from_numpy(ys + 0.5)], -1).to(f64)  # [m, 2]
                    a, bb = tri, tri.roll(-1, dims=1)                                 # edges a -> bb
                    e = bb - a
                    area = (e[:, 0, 0] * (tri[:, 2, 1] - tri[:, 0, 1]) - e[:, 0, 1] * (tri[:, 2, 0] - tri[:, 0, 0]))
                    sgn = th.where(area < 0, -1.0, 1.0).to(f64)
                    cross = e[None, :, :, 0] * (c[:, None, None, 1] - a[None, :, :, 1]) - e[None, :, :, 1] * (c[:, None, None, 0] - a[None, :, :, 0])
                    dist = cross * sgn[None, :, None] / th.sqrt((e * e).sum(-1)).clamp(min=1e-30)[None]  # [m, n, 3]
                    md = dist.min(-1).values
                    cov = (md > 0) & (area != 0)[None]
                    amb = (md.abs() < EDGE_EPS).any(1)
                    for i in range(len(xs)):
                        y, x = ys[i], xs[i]
                        nc = n_contrib[b, y, x]
                        ok = not bool(amb[i]) or nc == 0
                        # the walk: faces covered below n_contrib (the oracle's walk stops there)
                        idx = th.nonzero(cov[i, :nc]).reshape(-1)
                        if ok and nc > 0 and not bool(cov[i, nc - 1]):
                            ok = False
                        keep[b, y, x] = ok
                        if ok and idx.numel():
                            lists[(b, y, x)] = fl[idx]
                            K = max(K, idx.numel())
        # pixels with blended pairs: their faces in list order; clamp-border and n_contrib checks
        pix = sorted(lists)
        N = len(pix)
        self.faces_of = th.full((N, K), -1, dtype=th.int64)
        for i, k in enumerate(pix):
            self.faces_of[i, :lists[k].numel()] = lists[k]
        pix = np.array(pix, dtype=np.int64).reshape(-1, 3)
        self.view, self.py, self.px = (th.from_numpy(pix[:, j]) for j in range(3))
        self.keep = th.from_numpy(keep)
        if N:
            with th.no_grad():
                _, _, uvs, n_blend = self._walk({k: self.d[k].to(f64) for k in KEYS}, need_uv=True)
            bad = np.zeros(N, bool)
            for u, v, live in uvs:
                bad |= (live & (_clamp_border_dist(u, v) < CLAMP_EPS)).numpy()
            cnt = (self.faces_of >= 0).sum(1)
            # the oracle's walk ended where ours does: after the last covered face (T < T_EPS or the list's end)
            bad |= (n_blend != cnt).numpy()
            self.keep[pix[bad, 0], pix[bad, 1], pix[bad, 2]] = False
            sel = th.from_numpy(~bad)
            self.faces_of, self.view, self.py, self.px = self.faces_of[sel], self.view[sel], self.py[sel], self.px[sel]

    def _all_rays(self, mv, proj):
        B, H, W = self.B, self.H, self.W
        v, y, x = th.meshgrid(th.arange(B), th.arange(H), th.arange(W), indexing="ij")
        o, d = pixel_rays(mv, proj, v.reshape(-1), x.reshape(-1), y.reshape(-1), H, W)
        return o.reshape(B, H, W, 3), d.reshape(B, H, W, 3)

    @property
    def kept_fraction(self) -> float:
        return float(self.keep.sum()) / float(self.B * self.H * self.W)

    def mask(self) -> th.Tensor:
        """[B,1,H,W] float: 1 on kept pixels, 0 elsewhere (multiply both upstream gradients by it)."""
        return self.keep.to(th.float32).reshape(self.B, 1, self.H, self.W)

    def _walk(self, x: Dict[str, th.Tensor], need_uv: bool = False):
        faces = self.d["faces"].long()
        verts, vcol, fop, vdep, fint = x["verts"], x["verts_color"], x["faces_opacity"], x["verts_depth"], x["faces_intense"]
        o, d = pixel_rays(x["mv_mats"], x["proj_mats"], self.view, self.px, self.py, self.H, self.W)
        N, K = self.faces_of.shape
        C = th.zeros(N, 3, dtype=th.float64)
        D = th.zeros(N, dtype=th.float64)
        T = th.ones(N, dtype=th.float64)
        done = th.zeros(N, dtype=th.bool)
        n_blend = th.zeros(N, dtype=th.int64)
        uvs = []
        for k in range(K):
            live = (self.faces_of[:, k] >= 0) & ~done
            f = self.faces_of[:, k].clamp(min=0)
            i0, i1, i2 = faces[f, 0], faces[f, 1], faces[f, 2]
            u, v = _uv(o, d, verts[i0], verts[i1], verts[i2])
            if need_uv:
                uvs.append((u.detach(), v.detach(), live))
            uc, vc = _clamp(u, v)
            w0 = 1 - uc - vc
            col = (w0[:, None] * vcol[i0] + uc[:, None] * vcol[i1] + vc[:, None] * vcol[i2]) * fint[self.view, f][:, None]
            dep = w0 * vdep[self.view, i0] + uc * vdep[self.view, i1] + vc * vdep[self.view, i2]
            a = fop[f]
            wgt = th.where(live, a * T, th.zeros_like(a))
            C = C + wgt[:, None] * col
            D = D + wgt * dep
            T = th.where(live, T * (1 - a), T)
            n_blend = n_blend + live.long()
            done = done | (live & (T < T_EPS))
        return C, D, uvs, n_blend

    def render(self, x: Dict[str, th.Tensor]):
        """(color [N,3], depth [N]) of the kept pixels with blended pairs, from float64 leaves x (KEYS)."""
        C, D, _, _ = self._walk(x)
        # T after the walk: recomputed in _walk's order; background and the depth's "+ T"
        T = th.ones(C.shape[0], dtype=th.float64)
        done = th.zeros_like(T, dtype=th.bool)
        fop = x["faces_opacity"]
        for k in range(self.faces_of.shape[1]):
            live = (self.faces_of[:, k] >= 0) & ~done
            a = fop[self.faces_of[:, k].clamp(min=0)]
            T = th.where(live, T * (1 - a), T)
            done = done | (live & (T < T_EPS))
        bg = self.d["bg"].to(th.float64)
        return C + T[:, None] * bg[None], D + T

    def grads(self, gc: th.Tensor, gd: th.Tensor):
        """Gradients of sum(gc * color) + sum(gd * depth) over the kept pixels with blended pairs (gc [B,3,H,W],
        gd [B,1,H,W], already masked) in float64, and the forward (color [N,3], depth [N])."""
        leaves = {k: self.d[k].to(th.float64).clone().requires_grad_(True) for k in KEYS}
        color, depth = self.render(leaves)
        gcf = gc.to(th.float64)[self.view, :, self.py, self.px]
        gdf = gd.to(th.float64)[self.view, 0, self.py, self.px]
        ((color * gcf).sum() + (depth * gdf).sum()).backward()
        return {k: v.grad.numpy() for k, v in leaves.items()}, color.detach(), depth.detach()
