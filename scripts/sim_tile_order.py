"""CPU model behind the placed tile order (dmesh_renderer_amd/csrc/dmr_tile_order.hpp): what a tile -> XCD assignment means
for the mesh data one XCD's L2 sees, and for the makespan of a compositing kernel.  numpy only, no GPU.

    python scripts/sim_tile_order.py [--config C4]

1. Binning: the faces' tile rects as k_project_verts / face_bin compute them (float32 arithmetic, the double division and
   pixel mapping of dmr_device.hpp), counted per tile.  C4: R = 918 402 list entries in 2 916 busy tiles, the library's
   num_rendered.
2. Working set per class: workgroups are dealt round-robin over 8 XCDs, so the tiles at positions x, x + 8, ... of the
   order share an L2.  For each class the distinct 128-byte lines its tiles' faces touch in verts (12 B / vertex),
   verts_color (12 B), vproj (16 B), faces (12 B / face), opacity (4 B) and intensity (4 B).
3. Slot model: one queue per XCD in position order, 192 workgroup slots (32 CUs x 6), a busy tile holds its slot for
   6 + 9.6 us per 128-entry chunk, an empty one for nothing.  Reported: when the last tile of each XCD ends.

Orders compared: today's (global longest list first, position mod 8), 8 bands of tile rows (row-major inside a band: round
2's form; longest first inside a band), and blocks of n x n tiles dealt heaviest first to the least loaded class, longest
first inside a class (n = 4, 8, 16; the rule of dmr_tile_order.hpp, without blended pairs: cost = entries + 44)."""
import argparse
import heapq
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dmesh_renderer_amd import scenes  # noqa: E402

TILE, CLASSES, SLOTS, T_START, T_CHUNK, CHUNK = 16, 8, 192, 6.0, 9.6, 128
f32 = np.float32


def project(d, b, H, W):
    """vproj of view b as k_project_verts writes it: (pixel x, pixel y, NDC z), float32 operation by operation."""
    v = d["verts"].numpy().astype(f32)
    mv, pr = d["mv_mats"][b].numpy().astype(f32), d["proj_mats"][b].numpy().astype(f32)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    p = [mv[r, 0] * x + mv[r, 1] * y + mv[r, 2] * z + mv[r, 3] for r in range(3)]
    c = [pr[r, 0] * p[0] + pr[r, 1] * p[1] + pr[r, 2] * p[2] + pr[r, 3] for r in range(4)]
    w, eps = c[3].copy(), f32(1e-4)
    w[(w >= 0) & (w < eps)] = eps
    w[(w < 0) & (w > -eps)] = -eps
    pw = (1.0 / w.astype(np.float64)).astype(f32)
    n = [c[k] * pw for k in range(3)]
    px = (((n[0].astype(np.float64) + 1.0) * W - 1.0) * 0.5).astype(f32)
    py = (((n[1].astype(np.float64) + 1.0) * H - 1.0) * 0.5).astype(f32)
    return px, py, n[2]


def rects(d, b, H, W):
    """(minx, miny, maxx, maxy) tile rects of view b's faces (face_bin / tile_rect; empty for culled faces)."""
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    px, py, pz = project(d, b, H, W)
    f = d["faces"].numpy().astype(np.int64)
    X, Y, Z = px[f], py[f], pz[f]
    t = lambda a: np.trunc(a / f32(TILE)).astype(np.int64)
    minx, miny = np.clip(t(X.min(1)), 0, gx), np.clip(t(Y.min(1)), 0, gy)
    maxx, maxy = np.clip(t(X.max(1)) + 1, 0, gx), np.clip(t(Y.max(1)) + 1, 0, gy)
    maxy = np.maximum(maxy, miny)
    culled = (Z.max(1) < -1.0) | (Z.min(1) > 1.0)
    maxx[culled] = minx[culled]
    return minx, miny, np.maximum(maxx, minx), maxy


def bin_scene(d, B, H, W):
    """-> (entries per tile [B * gy * gx], (tile, face) pairs as two arrays)."""
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    tiles, faces = [], []
    for b in range(B):
        minx, miny, maxx, maxy = rects(d, b, H, W)
        w, h = maxx - minx, maxy - miny
        n = w * h
        fid = np.repeat(np.arange(n.size), n)
        k = np.arange(n.sum()) - np.repeat(np.cumsum(n) - n, n)
        tx, ty = minx[fid] + k % np.maximum(w[fid], 1), miny[fid] + k // np.maximum(w[fid], 1)
        tiles.append((b * gy + ty) * gx + tx)
        faces.append(fid)
    tiles, faces = np.concatenate(tiles), np.concatenate(faces)
    return np.bincount(tiles, minlength=B * gx * gy), tiles, faces


# ---- orders ---------------------------------------------------------------------------------------------------------------------
def order_global(count):
    return np.argsort(-count, kind="stable")


def positions(classes_of_busy, count):
    """Classes -> an order: class x's busy tiles take positions x, x + 8, ... longest first (or in the given sequence),
    empties fill the rest."""
    n = count.size
    order = np.full(n, -1, dtype=np.int64)
    room = [(n - x + CLASSES - 1) // CLASSES for x in range(CLASSES)]
    cls = [list(ts[:room[x]]) for x, ts in enumerate(classes_of_busy)]
    for x, ts in enumerate(classes_of_busy):  # a class with more busy tiles than positions spills its last ones
        for t in ts[room[x]:]:
            cls[int(np.argmax([room[y] - len(cls[y]) for y in range(CLASSES)]))].append(t)
    for x, ts in enumerate(cls):
        order[x + CLASSES * np.arange(len(ts))] = ts
    order[order < 0] = np.flatnonzero(count == 0)
    return order


def order_bands(count, B, gx, gy, longest_first):
    """8 bands of tile rows with equal total cost; row-major or longest first inside a band."""
    cost = np.where(count > 0, count + 44, 0).reshape(B * gy, gx).sum(1)
    edges = np.searchsorted(np.cumsum(cost), cost.sum() * np.arange(1, CLASSES) / CLASSES)
    band = np.searchsorted(edges, np.arange(B * gy), side="right")
    cls = []
    for x in range(CLASSES):
        ts = np.flatnonzero((np.repeat(band, gx) == x) & (count > 0))
        cls.append(ts[np.argsort(-count[ts], kind="stable")] if longest_first else ts)
    return positions(cls, count)


def order_blocks(count, B, gx, gy, blk):
    """dmr_tile_order.hpp without pairs and without spill."""
    t = np.arange(count.size)
    nbx, nby = (gx + blk - 1) // blk, (gy + blk - 1) // blk
    block = ((t // (gx * gy)) * nby + (t // gx) % gy // blk) * nbx + t % gx // blk
    cost = np.bincount(block, weights=np.where(count > 0, count + 44.0, 0.0), minlength=B * nbx * nby)
    load, home = np.zeros(CLASSES), np.zeros(cost.size, dtype=np.int64)
    for k in np.argsort(-cost, kind="stable"):
        if cost[k] > 0:
            home[k] = int(np.argmin(load))
            load[home[k]] += cost[k]
    cls = []
    for x in range(CLASSES):
        ts = np.flatnonzero((home[block] == x) & (count > 0))
        cls.append(ts[np.argsort(-count[ts], kind="stable")])
    return positions(cls, count), load


# ---- what an order costs -----------------------------------------------------------------------------------------------------
def working_set(order, tiles, faces, face_verts, B, P, F):
    """MB of distinct 128-byte lines per class."""
    cls_of_tile = np.empty(order.size, dtype=np.int64)
    cls_of_tile[order] = np.arange(order.size) % CLASSES
    pair_cls = cls_of_tile[tiles]
    view = tiles // (order.size // B)
    out = []
    for x in range(CLASSES):
        m = pair_cls == x
        f, b = faces[m], view[m]
        v = face_verts[f].reshape(-1)
        vb = np.repeat(b, 3)
        lines = 0
        lines += 2 * np.unique(np.concatenate([v * 12 // 128, (v * 12 + 11) // 128])).size  # verts and verts_color
        lines += np.unique((vb * P + v) * 16 // 128).size                                    # vproj
        lines += np.unique(np.concatenate([f * 12 // 128, (f * 12 + 11) // 128])).size      # faces
        lines += np.unique(f * 4 // 128).size + np.unique((b * F + f) * 4 // 128).size       # opacity, intensity
        out.append(lines * 128 / 1e6)
    return out


def makespan(order, count):
    """us at which each XCD's last tile ends."""
    ends = []
    for x in range(CLASSES):
        c = count[order[x::CLASSES]]
        slots = [0.0] * SLOTS
        heapq.heapify(slots)
        end = 0.0
        for n in c[c > 0]:
            t = heapq.heappop(slots) + T_START + T_CHUNK * -(-int(n) // CHUNK)
            end = max(end, t)
            heapq.heappush(slots, t)
        ends.append(end)
    return ends


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C4")
    a = ap.parse_args()
    cfg = scenes.CONFIGS[a.config]
    d = scenes.make(a.config)
    B, H, W = cfg.B, cfg.H, cfg.W
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    count, tiles, faces = bin_scene(d, B, H, W)
    fv = d["faces"].numpy().astype(np.int64)
    P, F = d["verts"].shape[0], fv.shape[0]
    print(f"{a.config}: {gx} x {gy} tiles x {B}, R = {int(count.sum())}, busy tiles {int((count > 0).sum())}, longest list {int(count.max())}, "
          f"mesh data {(P * (24 + 16 * B) + F * (16 + 4 * B)) / 1e6:.1f} MB")
    orders = [("global longest first (today)", order_global(count)),
              ("8 row bands, row-major", order_bands(count, B, gx, gy, False)),
              ("8 row bands, longest first", order_bands(count, B, gx, gy, True))]
    for blk in (4, 8, 16):
        o, load = order_blocks(count, B, gx, gy, blk)
        orders.append((f"blocks {blk} x {blk} (class loads within {100 * (load.max() - load.min()) / load.mean():.1f} %)", o))
    for name, o in orders:
        assert np.array_equal(np.sort(o), np.arange(count.size))
        ws, ms = working_set(o, tiles, faces, fv, B, P, F), makespan(o, count)
        print(f"{name:58s} lines per XCD {min(ws):5.1f}-{max(ws):5.1f} MB   XCDs end at {min(ms):5.1f}-{max(ms):5.1f} us")


if __name__ == "__main__":
    main()
