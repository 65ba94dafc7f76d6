"""Checks of the tet renderer's fragment lists (render_tets(fragments=K) -> face [B,K,H,W], bary [B,K,2,H,W], count [B,H,W]):
a float64 composite of such lists over the oracle Scene's inputs, the lists the float64 model of tests/tet_grad_ref.py
implies, and the checks against the CPU oracle's forward state.  Plain numpy / torch on the CPU; imported by
tests/test_tet_fragments_cpu.py and tests/test_tet_fragments_gpu.py (and usable on any source of fragments)."""
import numpy as np
import torch as th

from fragments_ref import band_rows
from tet_grad_ref import T_EPS, _hits

FWD_TOL = 1e-5   # the project's forward bound (tests/test_tet_parity_gpu.py, tests/test_alpha_gpu.py)


def _clamp_w(w):
    eps = 1e-4
    return np.where((w >= 0) & (w < eps), eps, np.where((w < 0) & (w > -eps), -eps, w))


def composite64(sc, face, bary):
    """float64 composite of tet fragment lists over the oracle Scene `sc` -> (color [B,3,H,W] with the background, depth
    [B,1,H,W] = D + T, T [B,H,W]).  Colour: the interpolated vertex colours times faces_intense; depth: the ndc depth (z over
    clamp_w(w)) of the hit point (1 - u - v) p0 + u p1 + v p2; T: the renderer's rule -- T (1 - o) behind a face of opacity
    o < 1, T_EPS / 10 behind one of opacity 1.  A pixel without fragments (an inactive one) gives the bare background, depth 1
    and T = 1 (alpha 0)."""
    B, K, H, W = face.shape
    used = face >= 0
    f = np.where(used, face, 0).astype(np.int64)
    o = np.where(used, sc.faces_opacity.astype(np.float64)[f], 0.0)
    vid = sc.faces.astype(np.int64)[f]                                               # [B,K,H,W,3]
    u, v = bary[:, :, 0].astype(np.float64), bary[:, :, 1].astype(np.float64)
    bw = np.stack([1.0 - u - v, u, v], -1)                                           # [B,K,H,W,3]
    bidx = np.arange(B)[:, None, None, None]
    col = (bw[..., None] * sc.verts_color.astype(np.float64)[vid]).sum(-2)           # [B,K,H,W,3]
    col = col * sc.faces_intense.astype(np.float64)[bidx, f][..., None]
    pt = (bw[..., None] * sc.verts.astype(np.float64)[vid]).sum(-2)                  # the hit point, [B,K,H,W,3]
    mv = sc.mv.astype(np.float64).reshape(B, 4, 4)[:, None, None, None]              # m[4 * col + row] -> [.., col, row]
    pr = sc.proj.astype(np.float64).reshape(B, 4, 4)[:, None, None, None]
    view = (pt[..., :, None] * mv[..., :3, :]).sum(-2) + mv[..., 3, :]               # [B,K,H,W,4]
    clip = (view[..., :3, None] * pr[..., :3, :]).sum(-2) + pr[..., 3, :]
    dep = clip[..., 2] / _clamp_w(clip[..., 3])
    C = np.zeros((B, H, W, 3))
    D = np.zeros((B, H, W))
    T = np.ones((B, H, W))
    for k in range(K):
        w = T * o[:, k]
        C += w[..., None] * col[:, k]
        D += w * dep[:, k]
        T = np.where(used[:, k], np.where(o[:, k] >= 1.0, T_EPS * 0.1, T * (1.0 - o[:, k])), T)
    color = C.transpose(0, 3, 1, 2) + T[:, None] * sc.bg.astype(np.float64)[None, :3, None, None]
    return color, (D + T)[:, None], T


def model_lists(ref, verts, faces):
    """The fragment lists of the pixels the float64 model (TetGradRef) keeps -- its faces_of[:, :steps] and the float64
    Moeller-Trumbore (u, v) of its rays on them -- as face [B,K,H,W], bary [B,K,2,H,W] (float64), count [B,H,W], K the
    longest march; every other pixel empty."""
    B, H, W = ref.B, ref.H, ref.W
    N, K = ref.faces_of.shape
    face = np.full((B * H * W, K), -1, np.int32)
    bary = np.zeros((B * H * W, K, 2))
    count = np.zeros(B * H * W, np.int32)
    verts, faces = verts.to(th.float64), faces.long()
    pix = ref.pix.numpy()
    for k in range(K):
        live = (k < ref.steps).numpy()
        f = ref.faces_of[:, k].clamp(min=0)
        _, u, v, _ = _hits(ref.ro, ref.rd, verts[faces[f, 0]], verts[faces[f, 1]], verts[faces[f, 2]])
        face[pix[live], k] = f.numpy()[live]
        bary[pix[live], k, 0], bary[pix[live], k, 1] = u.numpy()[live], v.numpy()[live]
    count[pix] = ref.steps.numpy()
    return (face.reshape(B, H, W, K).transpose(0, 3, 1, 2).copy(), bary.reshape(B, H, W, K, 2).transpose(0, 3, 4, 1, 2).copy(),
            count.reshape(B, H, W))


def hits32(ro, rd, p0, p1, p2):
    """(u, v) of ray_tri_hit (csrc/dmr_device.hpp) in numpy float32, operation for operation: the float32 noise of the formula."""
    f = np.float32
    ro, rd, p0, p1, p2 = (np.asarray(a, f) for a in (ro, rd, p0, p1, p2))
    cross = lambda a, b: np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                                   a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)
    dot = lambda a, b: a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]
    T, E1, E2 = ro - p0, p1 - p0, p2 - p0
    P, Q = cross(rd, E2), cross(T, E1)
    inv = f(1.0) / dot(P, E1)
    return dot(P, T) * inv, dot(Q, rd) * inv


def check_state(ost, face, bary, count, rows=(0, 0)):
    """Against the oracle's forward state, on the band's rows: count == n_contrib where is_active, else 0; slot 0 is
    first_face and slot count - 1 last_face (count <= K), exactly; unused slots are -1 / 0, used ones hold a face."""
    B, K, H, W = face.shape
    assert face.dtype == np.int32 and bary.dtype == np.float32 and count.dtype == np.int32
    assert bary.shape == (B, K, 2, H, W) and count.shape == (B, H, W)
    m = np.broadcast_to(band_rows(H, rows)[None, :, None], (B, H, W))
    nc = ost.get("n_contrib").astype(np.int64).reshape(B, H, W)
    act = ost.get("is_active").reshape(B, H, W) != 0
    assert np.array_equal(count[m], np.where(act, nc, 0)[m])
    stored = np.minimum(count, K)
    unused = np.arange(K)[None, :, None, None] >= stored[:, None]
    mk = np.broadcast_to(m[:, None], face.shape)
    assert (face[unused & mk] == -1).all() and (face[~unused & mk] >= 0).all()
    assert (bary[np.broadcast_to((unused & mk)[:, :, None], bary.shape)] == 0).all()
    has = m & (count > 0)
    assert np.array_equal(face[:, 0][has], ost.get("first_face").reshape(B, H, W)[has])
    fits = has & (count <= K)
    last = np.take_along_axis(face, np.maximum(stored - 1, 0)[:, None].astype(np.int64), axis=1)[:, 0]
    assert np.array_equal(last[fits], ost.get("last_face").reshape(B, H, W)[fits])
    return has


def check_composite(sc, ost, ocolor, odepth, face, bary, count, rows=(0, 0), tag=""):
    """composite64 of the fragments reproduces the oracle's colour, depth and final T (where active; 1 elsewhere) within
    FWD_TOL on the band's rows.  Needs count <= K everywhere.  Prints what it measured."""
    B, K, H, W = face.shape
    assert int(count.max()) <= K, (int(count.max()), K)
    m = band_rows(H, rows)
    color, depth, T = composite64(sc, face, bary)
    act = ost.get("is_active").reshape(B, H, W) != 0
    oT = np.where(act, np.exp(ost.get("final_T").astype(np.float64).reshape(B, H, W)), 1.0)  # (the tet state keeps log T)
    ec = float(np.abs(color - ocolor)[:, :, m].max())
    ed = float(np.abs(depth - odepth.reshape(B, 1, H, W))[:, :, m].max())
    et = float(np.abs(T - oT)[:, m].max())
    print(f"\n{tag}: tet fragments composite vs oracle: colour {ec:.2e}  depth {ed:.2e}  final T {et:.2e}  (longest march {int(count.max())}, K {K})")
    assert ec <= FWD_TOL and ed <= FWD_TOL and et <= FWD_TOL, (ec, ed, et)
