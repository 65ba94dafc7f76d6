"""Expected values of the alpha (coverage) output, from the CPU oracle alone (TEST INFRASTRUCTURE ONLY), and an
oracle-backed `_C` stand-in that serves `alpha=` over tests/oracle_C.py.

Two identities carry everything:
  * forward: alpha = 1 - T with T the oracle's `final_T` (tri) / exp(`final_T`) (tet: its state keeps the log), 0 where the
    oracle's tet `active` is 0 and outside the rendered tile rows;
  * backward: what an upstream g_a adds to dL_dfaces_opacity is the oracle's faces_opacity gradient of the COLOURLESS TWIN
    scene (verts_color = 0, bg = (1, 0, 0), so that color[:, 0] == T) for upstream dL_dcolor[:, 0] = -g_a, dL_ddepth = 0.
    By linearity the expectation for upstream (g_c, g_d, g_a) is oracle(scene; g_c, g_d) + oracle(twin; -g_a)["faces_opacity"];
    every other gradient is that of the call without g_a.
"""
from __future__ import annotations

import numpy as np
import torch as th

import oracle_C
from oracle import oracle as O

TILE = 16
kwargs_seen = []  # (function name, sorted keyword names) of every stand-in call


def band_mask(H: int, rows) -> np.ndarray:
    """[H] 1.0 in the pixel rows of the tile-row band `rows` ((0, 0): all rows)."""
    m = np.ones(H, dtype=np.float32)
    if tuple(rows) != (0, 0):
        m[:] = 0
        m[min(H, TILE * rows[0]):min(H, TILE * rows[1])] = 1
    return m


def expected_alpha(sc, st, tet: bool, rows=(0, 0), active=None) -> np.ndarray:
    """alpha [B,1,H,W] of the oracle's forward state `st` of scene `sc`."""
    T = st.get("final_T").astype(np.float32).reshape(sc.B, 1, sc.H, sc.W)
    if tet:
        T = np.exp(T)
    a = (np.float32(1.0) - T) * band_mask(sc.H, rows)[None, None, :, None]
    if tet:
        a = a * (np.asarray(active).reshape(sc.B, 1, sc.H, sc.W) > 0.5)
    return a.astype(np.float32)


def twin_scene(sc, rows=(0, 0)):
    """The colourless twin of an oracle Scene: verts_color = 0, bg = (1, 0, 0)."""
    return O.Scene(np.array([1, 0, 0], np.float32), sc.verts, sc.faces, np.zeros_like(sc.verts_color), sc.faces_opacity,
                   sc.mv, sc.proj, sc.inv_mv, sc.inv_proj, sc.verts_depth, sc.faces_intense, sc.H, sc.W,
                   tets=sc.tets, face_tets=sc.face_tets, tet_faces=sc.tet_faces,
                   ray_random_seed=int(sc.c.ray_random_seed), rows=rows)


def alpha_opacity_grad(sc, g_a, tet: bool, rows=(0, 0)) -> np.ndarray:
    """dL_dfaces_opacity [F] of an upstream g_a [B,1,H,W] on alpha: the twin's gradient for dL_dcolor[:, 0] = -g_a."""
    tw = twin_scene(sc, rows)
    g_a = np.asarray(g_a, dtype=np.float32).reshape(sc.B, sc.H, sc.W)
    gc = np.zeros((sc.B, 3, sc.H, sc.W), np.float32)
    gc[:, 0] = -g_a
    gd = np.zeros((sc.B, 1, sc.H, sc.W), np.float32)
    if tet:
        st = O.tet_forward(tw)[3]
        return O.tet_backward(tw, st, gc, gd)["faces_opacity"]
    st = O.tri_forward(tw)[2]
    return O.tri_backward(tw, st, gc, gd)["faces_opacity"]


# ---- the stand-in: oracle_C's four functions with the `alpha` keyword of dmesh_renderer_amd._C --------------------------
def _with_alpha(depth, a):
    return th.cat([depth, th.from_numpy(a)], dim=1)


def render_tris(*args, rows=(0, 0), **kw):
    kwargs_seen.append(("render_tris", sorted(kw)))
    alpha = kw.pop("alpha", False)
    assert not kw, kw
    out = oracle_C.render_tris(*args, rows=rows)
    if not alpha:
        return out
    sc, st = oracle_C._state(out[3])
    return (out[0], out[1], _with_alpha(out[2], expected_alpha(sc, st, False, rows)), *out[3:])


def render_tris_backward(*args, rows=(0, 0), **kw):
    kwargs_seen.append(("render_tris_backward", sorted(kw)))
    alpha = kw.pop("alpha", False)
    assert not kw, kw
    if not alpha:
        return oracle_C.render_tris_backward(*args, rows=rows)
    args = list(args)
    gd = args[12]
    assert gd.dim() == 4 and gd.size(1) == 2, "alpha=True: dL_dout_depth must be [B,2,H,W]"
    args[12] = gd[:, :1]
    g = list(oracle_C.render_tris_backward(*args, rows=rows))
    sc, _ = oracle_C._state(args[14])
    g[2] = g[2] + th.from_numpy(alpha_opacity_grad(sc, gd[:, 1:].detach().contiguous().numpy(), False, rows))
    return tuple(g)


def render_tets(*args, rows=(0, 0), **kw):
    kwargs_seen.append(("render_tets", sorted(kw)))
    alpha = kw.pop("alpha", False)
    assert not kw, kw
    out = oracle_C.render_tets(*args, rows=rows)
    if not alpha:
        return out
    sc, st = oracle_C._state(out[3])
    return (out[0], _with_alpha(out[1], expected_alpha(sc, st, True, rows, out[2].numpy())), *out[2:])


def render_tets_backward(*args, rows=(0, 0), **kw):
    kwargs_seen.append(("render_tets_backward", sorted(kw)))
    alpha = kw.pop("alpha", False)
    assert not kw, kw
    if not alpha:
        return oracle_C.render_tets_backward(*args, rows=rows)
    args = list(args)
    gd = args[15]
    assert gd.dim() == 4 and gd.size(1) == 2, "alpha=True: grad_depth must be [B,2,H,W]"
    args[15] = gd[:, :1]
    g = list(oracle_C.render_tets_backward(*args, rows=rows))
    sc, _ = oracle_C._state(args[16])
    g[1] = g[1] + th.from_numpy(alpha_opacity_grad(sc, gd[:, 1:].detach().contiguous().numpy(), True, rows))
    return tuple(g)
