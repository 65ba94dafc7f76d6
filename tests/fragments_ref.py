"""Checks of the tri renderer's fragment lists (render_tris(fragments=K) -> face [B,K,H,W], bary [B,K,2,H,W], count [B,H,W])
against the CPU oracle's forward state and against the float64 model of tests/tri_grad_ref.py.  Plain numpy / torch on the
CPU; imported by tests/test_fragments_gpu.py (and usable on any source of fragments)."""
import numpy as np
import torch as th

from tri_grad_ref import _clamp, _uv

FWD_TOL = 1e-5   # the project's forward bound (tests/test_alpha_gpu.py, tests/test_tri_parity_gpu.py)


def band_rows(H, rows):
    """[H] bool: the pixel rows of the tile-row band (all rows for (0, 0))."""
    m = np.ones(H, bool)
    if tuple(rows) != (0, 0):
        m[:] = False
        m[16 * rows[0]:min(H, 16 * rows[1])] = True
    return m


def composite64(sc, face, bary, strip=128):
    """float64 composite of fragments over the oracle Scene's inputs -> (color [B,3,H,W] with the background, depth
    [B,1,H,W] = D + T, T [B,H,W]).  (In strips of rows: the intermediates are [B,K,rows,W,3,3] doubles.)"""
    H = face.shape[2]
    if H > strip:
        parts = [composite64(sc, face[:, :, y:y + strip], bary[:, :, :, y:y + strip], strip) for y in range(0, H, strip)]
        return tuple(np.concatenate([p[i] for p in parts], axis=-2) for i in range(3))
    B, K, H, W = face.shape
    used = face >= 0
    f = np.where(used, face, 0).astype(np.int64)
    fop = sc.faces_opacity.astype(np.float64)
    o = np.where(used, fop[f], 0.0)
    t = np.concatenate([np.ones((B, 1, H, W)), np.cumprod(1.0 - o, axis=1)], axis=1)
    w = o * t[:, :-1]
    vid = sc.faces.astype(np.int64)[f]                       # [B,K,H,W,3]
    u, v = bary[:, :, 0].astype(np.float64), bary[:, :, 1].astype(np.float64)
    bw = np.stack([1.0 - u - v, u, v], -1)                   # [B,K,H,W,3]
    bidx = np.arange(B)[:, None, None, None]
    col = (bw[..., None] * sc.verts_color.astype(np.float64)[vid]).sum(-2)          # [B,K,H,W,3]
    col = col * sc.faces_intense.astype(np.float64)[bidx, f][..., None]
    dep = (bw * sc.verts_depth.astype(np.float64)[bidx[..., None], vid]).sum(-1)    # [B,K,H,W]
    T = t[:, -1]
    color = (w[..., None] * col).sum(1).transpose(0, 3, 1, 2) + T[:, None] * sc.bg.astype(np.float64)[None, :3, None, None]
    depth = (w * dep).sum(1)[:, None] + T[:, None]
    return color, depth, T


def check_composite(sc, ost, ocolor, odepth, face, bary, count, rows=(0, 0), state=True, tag=""):
    """The float64 composite of the fragments reproduces the oracle's colour, its depth D + T and (state) final_T within
    FWD_TOL on the band's rows.  Needs count <= K everywhere.  Prints what it measured."""
    B, K, H, W = face.shape
    assert int(count.max()) <= K, (int(count.max()), K)
    m = band_rows(H, rows)
    color, depth, T = composite64(sc, face, bary)
    ec = float(np.abs(color - ocolor)[:, :, m].max())
    ed = float(np.abs(depth - odepth)[:, :, m].max())
    et = float(np.abs(T - ost.get("final_T").reshape(B, H, W))[:, m].max()) if state else 0.0
    print(f"\n{tag}: fragments composite vs oracle: colour {ec:.2e}  depth {ed:.2e}  final_T {et:.2e}  (deepest pixel {int(count.max())}, K {K})")
    assert ec <= FWD_TOL and ed <= FWD_TOL and et <= FWD_TOL, (ec, ed, et)


def check_lists(sc, ost, face, bary, count, rows=(0, 0)):
    """count == 0 exactly where n_contrib == 0; a pixel's fragment faces are an ordered subsequence of the first n_contrib
    entries of its tile's list, the last one the entry at n_contrib - 1; unused slots are -1 / 0.  Band rows only."""
    B, K, H, W = face.shape
    gx, gy = (W + 15) // 16, (H + 15) // 16
    ranges = ost.get("ranges").astype(np.int64).reshape(-1, 2)
    values = ost.get("values").astype(np.int64)
    nc = ost.get("n_contrib").astype(np.int64).reshape(B, H, W)
    m = band_rows(H, rows)
    assert np.array_equal((count == 0)[:, m], (nc == 0)[:, m])
    assert int(count.max()) <= K
    slot = np.arange(K)[None, :, None, None]
    unused = slot >= count[:, None]
    assert (face[unused & m[None, None, :, None]] == -1).all() and (face[~unused & m[None, None, :, None]] >= 0).all()
    assert (bary[np.broadcast_to(unused[:, :, None], bary.shape) & m[None, None, None, :, None]] == 0).all()
    for b, y, x in zip(*np.nonzero((nc > 0) & m[None, :, None])):
        r0 = ranges[(b * gy + y // 16) * gx + x // 16, 0]
        lst = values[r0:r0 + nc[b, y, x]]
        fr = face[b, :count[b, y, x], y, x]
        assert fr[-1] == lst[-1], (b, y, x)
        it = iter(lst)
        assert all(any(v == f for v in it) for f in fr), ("not an ordered subsequence of the tile's list", b, y, x)


def check_model(ref, d, face, bary, count, rows=(0, 0)):
    """On the pixels the float64 model (TriGradRef) keeps: the fragment faces equal its faces_of row for row, exactly, and
    bary equals its clamped Moeller-Trumbore (u, v) within FWD_TOL; kept pixels without a row blended nothing."""
    B, K, H, W = face.shape
    m = th.from_numpy(band_rows(H, rows))
    sel = m[ref.py]
    view, py, px, faces_of = ref.view[sel], ref.py[sel], ref.px[sel], ref.faces_of[sel]
    N, Kr = faces_of.shape
    assert N > 0 and Kr <= K
    want = th.full((N, K), -1, dtype=th.int64)
    want[:, :Kr] = faces_of
    got = th.from_numpy(face.astype(np.int64))[view, :, py, px]
    assert th.equal(got, want), int((got != want).any(1).sum())
    assert th.equal(th.from_numpy(count.astype(np.int64))[view, py, px], (faces_of >= 0).sum(1))
    none = ref.keep.clone()
    none[view, py, px] = False
    none &= m[None, :, None]
    assert (th.from_numpy(count)[none] == 0).all()
    verts, faces = d["verts"].to(th.float64), d["faces"].long()
    o, dr = ref.ray_o[view, py, px], ref.ray_d[view, py, px]
    gb = th.from_numpy(bary.astype(np.float64))[view, :, :, py, px]  # [N,K,2]
    err = 0.0
    for k in range(Kr):
        live = faces_of[:, k] >= 0
        f = faces_of[:, k].clamp(min=0)
        uc, vc = _clamp(*_uv(o, dr, verts[faces[f, 0]], verts[faces[f, 1]], verts[faces[f, 2]]))
        e = th.maximum((gb[:, k, 0] - uc).abs(), (gb[:, k, 1] - vc).abs())[live]
        err = max(err, float(e.max()) if e.numel() else 0.0)
    print(f"\nfragments vs the float64 model: {N} pixels with pairs, faces exact, bary {err:.2e}")
    assert err <= FWD_TOL, err
