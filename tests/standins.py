"""Recording stand-ins for `_C` in the CPU tests of the Python plumbing (test_tet_full_grads_cpu, test_tet_camera_grads_cpu,
test_tri_exact_grads_cpu): fixed forward outputs, the backward's arguments recorded, gradients in the order `_C` returns them."""
import torch as th


class _FakeC:
    """Records the render_tets_backward calls; returns recognisable gradients."""

    def __init__(self):
        self.calls = []

    def render_tets(self, bg, verts, faces, vcol, fop, mv, proj, imv, iproj, vdepth, fint, tets, ft, tf, H, W, seed, rows=(0, 0)):
        B = mv.shape[0]
        z = th.zeros(1)
        return th.zeros(B, 3, H, W), th.zeros(B, 1, H, W), th.ones(B, H, W), z, z, z, z

    def render_tets_backward(self, *args, **kw):
        self.calls.append((len(args), dict(kw)))
        verts, faces, mv, fint = args[1], args[2], args[5], args[10]
        P, F, B = verts.shape[0], faces.shape[0], mv.shape[0]
        g = (th.full((P, 3), 1.0), th.full((P, 3), 2.0), th.full((F,), 3.0), th.full(tuple(fint.shape), 4.0))
        if kw.get("camera_grads"):
            return g + (th.zeros(B, 4, 4), th.zeros(B, 4, 4), th.full((B, 4, 4), 5.0), th.full((B, 4, 4), 6.0))
        return g if kw.get("full_grads") else g[1:3]


class _StandIn:
    """`_C` stand-in: fixed outputs, records the keywords of render_tris_backward, returns given inverse gradients."""

    def __init__(self, B, P, F, H, W, g_inv):
        self.B, self.P, self.F, self.H, self.W, self.g_inv = B, P, F, H, W, g_inv
        self.kw = []

    def render_tris(self, bg, verts, faces, vc, fo, mv, proj, imv, iproj, vd, fi, H, W, rows=(0, 0)):
        e = th.zeros(1, dtype=th.uint8)
        return 1, th.zeros(self.B, 3, H, W, dtype=verts.dtype), th.zeros(self.B, 1, H, W, dtype=verts.dtype), e, e, e, e

    def render_tris_backward(self, *args, rows=(0, 0), **kw):
        self.kw.append(kw)
        B, P, F = self.B, self.P, self.F
        z = lambda *s: th.zeros(*s, dtype=th.float64)
        g = (z(P, 3), z(P, 3), z(F), z(B, P), z(B, F))
        return g + tuple(self.g_inv) if kw.get("camera_grads") else g
