"""Independent float64 reference for the tet renderer's full gradients (TetRenderer(full_grads=True)).

No march: every selected pixel's ray (the CPU oracle's ray_o / ray_d, promoted to float64) is intersected with EVERY
face of a convex mesh (scenes.kuhn_tets).  The strictly-inside hits, sorted by t, are the faces the ray crosses; the first
n_contrib of them are composited in log-T form as the oracle's tet_render_pixel does (opacity == 1 ends the march at
T = T_EPS / 10, T < T_EPS ends it).  Everything is differentiable in verts, verts_color, faces_opacity and
faces_intense, so torch.autograd gives the gradients -- the hit (t, u, v) of a ray on a face is a function of the three
vertices (Moeller-Trumbore), no chain rule is written by hand.

Only pixels where the brute force is unambiguous are kept: active in the oracle's forward, first and n_contrib-th hit
are the oracle's first_face / last_face, and there are at least n_contrib hits.  Also dropped: rays that pass within
EDGE_EPS (barycentric) of an edge of any face they cross.  Those are the rays along which the reference's reverse march
finds two candidate faces in one tet and stops before reaching first_face (backward.cu:456-460; the renderer under test
stops there too), so that the faces in front of the stop get no gradient.  In scenes.kuhn_tets the un-jittered boundary
vertices put whole rows of pixel rays into the planes of boundary faces.  The upstream gradients of all other pixels
are zeroed (`mask`), for the reference and for the renderer under test alike.
"""
from __future__ import annotations

from typing import Dict

import numpy as np
import torch as th

T_EPS = 1e-4  # auxiliary.h:8
KEYS = ("verts", "verts_color", "faces_opacity", "faces_intense")
EDGE_EPS = 1e-3


def _clamp_w(w):
    eps = 1e-4
    return th.where((w >= 0) & (w < eps), th.full_like(w, eps), th.where((w < 0) & (w > -eps), th.full_like(w, -eps), w))


def _hits(o, d, p0, p1, p2):
    """(t, u, v) of rays o, d [..., 3] on triangles p0, p1, p2 [..., 3] (broadcast), and den = (d x E2) . E1."""
    E1, E2 = p1 - p0, p2 - p0
    d, E1, E2, T = th.broadcast_tensors(d, E1, E2, o - p0)
    P = th.cross(d, E2, dim=-1)
    den = (P * E1).sum(-1)
    Q = th.cross(T, E1, dim=-1)
    t = (Q * E2).sum(-1) / den
    u = (P * T).sum(-1) / den
    v = (Q * d).sum(-1) / den
    return t, u, v, den


class TetGradRef:
    """Selection and float64 forward / gradients of one scene.  d: scenes.kuhn_tets dict; st: the oracle's tet_forward
    state of the same scene (rays, first / last face, n_contrib, is_active)."""

    def __init__(self, d: Dict[str, th.Tensor], H: int, W: int, st, chunk: int = 1024):
        self.d, self.H, self.W = d, H, W
        B = d["mv_mats"].shape[0]
        self.B = B
        f64 = th.float64
        ro = th.from_numpy(st.get("ray_o").reshape(B * H * W, 3)).to(f64)
        rd = th.from_numpy(st.get("ray_d").reshape(B * H * W, 3)).to(f64)
        first = th.from_numpy(st.get("first_face").astype(np.int64))
        last = th.from_numpy(st.get("last_face").astype(np.int64))
        n_contrib = th.from_numpy(st.get("n_contrib").astype(np.int64))
        active = th.from_numpy(st.get("is_active").astype(bool)) & (n_contrib > 0)
        verts = d["verts"].to(f64)
        faces = d["faces"].long()
        p0, p1, p2 = verts[faces[:, 0]], verts[faces[:, 1]], verts[faces[:, 2]]
        cand = th.nonzero(active).reshape(-1)
        K = int(n_contrib[cand].max()) if cand.numel() else 1
        keep = th.zeros(B * H * W, dtype=th.bool)
        order = th.full((B * H * W, K), -1, dtype=th.int64)
        with th.no_grad():
            for c0 in range(0, cand.numel(), chunk):
                idx = cand[c0:c0 + chunk]
                t, u, v, _ = _hits(ro[idx, None], rd[idx, None], p0[None], p1[None], p2[None])  # [n, F]
                inside = (u > 0) & (v > 0) & (u + v < 1) & (t > 0)
                bary = th.minimum(th.minimum(u, v), 1 - u - v)
                near_edge = ((bary > -EDGE_EPS) & (bary < EDGE_EPS) & (t > 0)).any(1)
                key = th.where(inside, t, th.full_like(t, float("inf")))
                srt = th.argsort(key, dim=1)[:, :K]
                cnt = inside.sum(1)
                nc = n_contrib[idx]
                srt = th.where(th.arange(K)[None] < cnt[:, None].clamp(max=K), srt, th.full_like(srt, -1))
                ok = (cnt >= nc) & (srt[:, 0] == first[idx]) & ~near_edge
                ok &= srt.gather(1, (nc - 1).clamp(min=0)[:, None])[:, 0] == last[idx]
                keep[idx] = ok
                order[idx] = srt
        self.n_active = int(active.sum())
        self.keep = keep                                       # [B*H*W]
        self.pix = th.nonzero(keep).reshape(-1)                # kept pixels, flat b*H*W + y*W + x
        self.faces_of = order[self.pix]                        # [N, K], -1 past the hits
        self.steps = n_contrib[self.pix]                       # [N]
        self.ro, self.rd = ro[self.pix], rd[self.pix]
        self.view = self.pix // (H * W)

    @property
    def kept_fraction(self) -> float:
        return self.pix.numel() / max(1, self.n_active)

    def mask(self) -> th.Tensor:
        """[B,1,H,W] float: 1 on kept pixels, 0 elsewhere (multiply both upstream gradients by it)."""
        return self.keep.to(th.float32).reshape(self.B, 1, self.H, self.W)

    def render(self, inputs: Dict[str, th.Tensor]):
        """Composited (color [N,3], depth [N]) of the kept pixels from float64 leaves `inputs` (KEYS)."""
        d = self.d
        verts, vcol, fop, fint = (inputs[k] for k in KEYS)
        faces = d["faces"].long()
        bg = d["bg"].to(th.float64)
        mv = d["mv_mats"].to(th.float64)[self.view]       # [N,4,4] row-major: view = M @ (p, 1)
        pr = d["proj_mats"].to(th.float64)[self.view]
        N, K = self.faces_of.shape
        C = th.zeros(N, 3, dtype=th.float64)
        D = th.zeros(N, dtype=th.float64)
        log_T = th.zeros(N, dtype=th.float64)
        fT = th.ones(N, dtype=th.float64)                     # T after the pixel's last step
        for k in range(K):
            live = k < self.steps                              # [N]
            f = self.faces_of[:, k].clamp(min=0)
            i0, i1, i2 = faces[f, 0], faces[f, 1], faces[f, 2]
            t, u, v, _ = _hits(self.ro, self.rd, verts[i0], verts[i1], verts[i2])
            col = vcol[i0] + (vcol[i1] - vcol[i0]) * u[:, None] + (vcol[i2] - vcol[i0]) * v[:, None]
            col = col * fint[self.view, f][:, None]
            a = fop[f]
            T = th.exp(log_T)
            X = self.ro + t[:, None] * self.rd
            vp = (mv[:, :3, :3] @ X[:, :, None])[:, :, 0] + mv[:, :3, 3]
            cz = (pr[:, 2, :3] * vp).sum(-1) + pr[:, 2, 3]
            cw = (pr[:, 3, :3] * vp).sum(-1) + pr[:, 3, 3]
            pdepth = cz / _clamp_w(cw)
            w = th.where(live, T * a, th.zeros_like(a))
            C = C + w[:, None] * col
            D = D + w * pdepth
            opaque = a >= 1.0
            new_log_T = th.where(opaque, th.full_like(log_T, float(np.log(np.float32(T_EPS * 0.1)))),
                                 log_T + th.log1p(-th.where(opaque, th.zeros_like(a), a)))
            # the reference's backward treats an opaque face's final T as T * (1 - opacity) (its value is T_EPS / 10)
            T_next = th.where(opaque, T * (1 - a) - (T * (1 - a)).detach() + T_EPS * 0.1, th.exp(new_log_T))
            log_T = th.where(live, new_log_T, log_T)
            fT = th.where(live, T_next, fT)
        color = C + fT[:, None] * bg[None]
        depth = D + fT
        return color, depth

    def grads(self, gc: th.Tensor, gd: th.Tensor):
        """Gradients of sum(gc * color) + sum(gd * depth) over the kept pixels (gc [B,3,H,W], gd [B,1,H,W]) in float64,
        and the forward (color [N,3], depth [N])."""
        leaves = {k: self.d[k].to(th.float64).clone().requires_grad_(True) for k in KEYS}
        color, depth = self.render(leaves)
        HW = self.H * self.W
        b, r = self.view, self.pix % HW
        gcf = gc.to(th.float64).reshape(self.B, 3, HW)[b, :, r]   # [N,3]
        gdf = gd.to(th.float64).reshape(self.B, HW)[b, r]
        ((color * gcf).sum() + (depth * gdf).sum()).backward()
        return {k: v.grad.numpy() for k, v in leaves.items()}, color.detach(), depth.detach()
