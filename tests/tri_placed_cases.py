"""The tri renderer's PLACED front end (k_project_verts with SegInit -> k_bin_faces -> k_tri_forward, dmr_api.hip "Speculative
PLACEMENT"): the scene pairs that send it down every emission route of bin_emit<FPT, true>, and the classifier that says, from
the CPU oracle's state alone, which route every list entry takes and which tiles leave their segment.

A pair is (A, B): the placement is built from a default call of A, B is binned into it.  classify() restates bin_emit
(dmr_binning.hip) on the oracle's lists: a workgroup takes 256 * FPT consecutive (view, face) pairs, its window's view is its
first pair's; a face goes
    window        its own view's, not big: counted in the LDS histogram, ONE reservation per (workgroup, tile), accepted as a
                  whole or not at all (first + c <= limit);
    cooperative   big (touched > BIG_RECT) and queued: emitted by the whole workgroup, a slot at a time, slot < limit;
    direct        another view's face, or a big face beyond the BIG_MAX the queue holds: its own thread, slot < limit;
with limit = min(seg[t + 1], capacity) per tile.  Which BIG_MAX of more big faces are queued is decided by an LDS atomic, so a
workgroup with more than BIG_MAX of them has `big_mixed` entries: BIG_MAX faces' worth cooperative, the others' direct.
(A frame the placed path takes has at most SCAN_SINGLE_MAX = LDS_HIST_MAX tiles, so a workgroup with a window face always has
a window.)

FITTING pairs: B is A with every vertex moved by up to JITTER_PX pixels; no tile of B leaves the segment A's count gives it.
OVERFLOW pairs: B is A with a stack of faces brought into the frame (in A they lie beyond the far plane, so F is equal); every
tile either keeps A's list exactly or leaves its segment -- no tile gains entries and still fits, so the backward's record
buffer, sized from A's pairs, cannot overflow.

The view configurations (B, H, W, rows) of this file, each used by no other tri call of the suite (placements and size
estimates are keyed by them; tests/test_tri_placed_paths_cpu.py checks the list against the other test files' text):
    (1, 336, 320)  big_queue            (2, 112, 176)  behind_camera      (1, 48, 32)    bitonic_in_segments
    (1, 2048, 1024) tiles_8192          (3, 176, 208)  straddle           (3, 64, 48)    fpt2
    (11, 32, 64)   fpt4                 (1, 208, 240) rows (3, 9)  band
    (1, 160, 208)  over_window          (1, 512, 496)  over_cooperative   (1, 496, 512)  over_direct_big
    (2, 176, 224)  over_direct_view
"""
import math

import numpy as np
import torch as th

from dmesh_renderer_amd import scenes
from tet_cases import SORT_LDS_KEYS, bin_fpt, sort_path  # noqa: F401  (the sort's constants and rule: restated there, once)
from util import upstream_grads, with_bg

# ---- what the kernels decide by, restated (test_tri_placed_paths_cpu.py checks each against the sources' text) ---------------
SEG_SLACK = 32            # dmr_kernels.hpp: entries a segment has room for beyond count + 25 %
BIG_RECT = 256            # dmr_binning.hip: a face whose rect covers more tiles is emitted by the whole workgroup
BIG_MAX = 128             # dmr_binning.hip: ... while its workgroup's queue has room
LDS_HIST_MAX = 8192       # dmr_binning.hip: tiles a workgroup's window may cover
FPT_2, FPT_4 = 256 * 1024, 1024 * 1024   # dmr_binning.hip, bin_fpt
SCAN_SINGLE_MAX = 8192    # dmr_kernels.hpp: frames up to here are placed
MASK_CHUNK = 128          # dmr_kernels.hpp: list entries per coverage-mask slot and per compositing chunk
TILE = 16
ROUTES = ("window", "cooperative", "direct", "big_mixed")


def seg_len(c):
    """k_build_placement: the segment of a tile that held c entries."""
    return c + (c >> 2) + SEG_SLACK


def placed_capacity(R, ntiles):
    """dmr_api.hip, placement_capacity: what an asynchronous placed call returns in R's place."""
    return R + R // 4 + SEG_SLACK * ntiles


def size_bucket(n):
    """dmr_api.hip: floor(log2(B * F)), part of the placement's key."""
    return max(int(n).bit_length() - 1, 0)


# ---- the scenes --------------------------------------------------------------------------------------------------------------
JITTER_PX = 1.0
LOW = (0.01, 0.1)   # the opacity of the long-list cases, as the tet fpt cases': T stays far from the early-out threshold


def pixel(H):
    """world units per pixel at the cameras' distance (radius 3, fovy 60 degrees)"""
    return 2.0 * 3.0 * math.tan(math.radians(30.0)) / H


def jittered(d, H, seed, px=JITTER_PX):
    """d with every vertex coordinate moved by up to +- px pixels (verts_depth, an input attribute only, stays)"""
    g = th.Generator().manual_seed(seed)
    return dict(d, verts=d["verts"] + (th.rand(d["verts"].shape, generator=g) * 2.0 - 1.0) * (px * pixel(H)))


def _sheets(L, n, B, H, W, seed, opacity=(0.1, 0.5), scale=(1.0, 1.0, 1.0), shift=(0.0, 0.0, 0.0)):
    d = scenes.layered_sheets(L, n, B, H, W, seed=seed, opacity=opacity)
    d["verts"] = d["verts"] * th.tensor(scale) + th.tensor(shift)
    return d


def _big_queue(B, H, W):
    """many_big's shape -- 300 consecutive two-triangle sheets far larger than their mesh -- with the sheets' half width
    growing from 1.0 to 6: the small ones end inside the frame (tile counts differ over the frame and move with the jitter),
    all but a few cover more than BIG_RECT tiles."""
    d = scenes.layered_sheets(150, 2, B, H, W, seed=0, opacity=(0.005, 0.02))
    s = th.linspace(1.0, 6.0, 150).repeat_interleave(4)
    d["verts"] = d["verts"] * th.stack([s, s, th.ones_like(s)], 1)
    return d


FIT = {
    # name: (B, H, W, rows, background, scene)
    "big_queue": (1, 336, 320, (0, 0), False, lambda B, H, W: _big_queue(B, H, W)),
    # vertices far off screen and behind the eye plane (test_tri_parity_gpu's `huge`)
    "behind_camera": (2, 112, 176, (0, 0), False, lambda B, H, W: _sheets(3, 8, B, H, W, 0, (0.1, 0.4), (6.0, 6.0, 4.5))),
    # 5 120 faces over six tiles: lists beyond SORT_LDS_KEYS -- the bitonic network inside a padded segment, dozens of mask chunks
    "bitonic_in_segments": (1, 48, 32, (0, 0), False, lambda B, H, W: _sheets(40, 9, B, H, W, 0, LOW)),
    # exactly SCAN_SINGLE_MAX tiles, a small mesh: k_build_placement's slab and the size workgroup's loop full
    "tiles_8192": (1, 2048, 1024, (0, 0), False, lambda B, H, W: _sheets(3, 24, B, H, W, 5, (0.1, 0.5), (0.5, 0.5, 1.0))),
    # three views, F = 726: workgroups hold pairs of two views
    "straddle": (3, 176, 208, (0, 0), True, lambda B, H, W: _sheets(3, 12, B, H, W, 2)),
    "fpt2": (3, 64, 48, (0, 0), False, lambda B, H, W: _sheets(6, 87, B, H, W, 0, LOW)),       # 88 752 faces a view: 266 256 pairs
    "fpt4": (11, 32, 64, (0, 0), False, lambda B, H, W: _sheets(6, 91, B, H, W, 0, LOW)),      # 97 200 a view: 1 069 200 pairs
    # a band of tile rows of a frame the mesh overfills: faces cross both of the band's edges
    "band": (1, 208, 240, (3, 9), False, lambda B, H, W: _sheets(3, 20, B, H, W, 4, (0.1, 0.5), (2.6, 2.6, 1.0))),
}
ASYNC_TOO = ("big_queue", "bitonic_in_segments")   # ... whose B call is also made asynchronously


def fit_pair(name):
    """-> (A, B, (B, H, W), rows)"""
    B, H, W, rows, bg, make = FIT[name]
    a = make(B, H, W)
    if bg:
        a = with_bg(a)
    return a, jittered(a, H, 77), (B, H, W), rows


FAR_Z = -20.0   # beyond the far plane of every camera in front of it: culled


def _cat(parts):
    """one mesh of several (the first part's cameras and background)"""
    d = dict(parts[0])
    off, faces = 0, []
    for p in parts:
        faces.append(p["faces"] + off)
        off += p["verts"].shape[0]
    d["faces"] = th.cat(faces)
    for k in ("verts", "verts_color", "faces_opacity"):
        d[k] = th.cat([p[k] for p in parts])
    for k in ("verts_depth", "faces_intense"):
        d[k] = th.cat([p[k] for p in parts], dim=1)
    return d


def _stack(B, H, W, copies, x0, x1, y0, y1, seed):
    """`copies` copies of one quad (two triangles) [x0, x1] x [y0, y1] at z = 0.3, faint"""
    q = scenes.layered_sheets(1, 2, B, H, W, seed=seed, opacity=(0.005, 0.02))
    q["verts"] = th.tensor([[x0, y0, 0.3], [x1, y0, 0.3], [x0, y1, 0.3], [x1, y1, 0.3]])
    d = _cat([q] * copies)
    return d


# name: (B, H, W, copies, the stack's quad (x0, x1, y0, y1), what lies in the frame besides, the route the case is for)
OVER = {
    # a quad of a few tiles, 48 times: 96 small faces of the one view in one workgroup -- window reservations that do not fit
    "over_window": (1, 160, 208, 48, (-1.1, -0.35, -0.45, 0.5), "window"),
    # a quad over the left half of a frame of 992 tiles, 40 times: 80 big faces, all queued
    "over_cooperative": (1, 512, 496, 40, (-1.6, -0.1, -1.55, 1.55), "cooperative"),
    # the same 80 times: 160 big faces in the first workgroup, 32 beyond the queue
    "over_direct_big": (1, 496, 512, 80, (-1.6, -0.1, -1.55, 1.55), "big_mixed"),
    # two views, the stack first in the face array: the workgroup that straddles the view border emits view 1's copies directly
    "over_direct_view": (2, 176, 224, 48, (-1.1, -0.35, -0.45, 0.5), "direct"),
}


def over_pair(name):
    """-> (A, B, (B, H, W), rows).  The frame: dense sheets over the right half (untouched, long lists), sparse sheets over
    the left half (some tiles busy, some empty), and the stack over a part of the left half -- first in the face array, at
    z = FAR_Z in A."""
    B, H, W, copies, (x0, x1, y0, y1), _ = OVER[name]
    stack = _stack(B, H, W, copies, x0, x1, y0, y1, 31)
    dense = _sheets(6, 24, B, H, W, 32, (0.1, 0.5), (0.75, 1.6, 1.0), (0.95, 0.0, 0.0))
    sparse = _sheets(2, 7, B, H, W, 33, (0.1, 0.5), (0.55, 0.8, 1.0), (-0.75, -0.6, 0.0))
    b = _cat([stack, dense, sparse])
    a = dict(b, verts=b["verts"].clone())
    a["verts"][: 4 * copies, 2] = FAR_Z
    return a, b, (B, H, W), (0, 0)


def pair(name):
    return fit_pair(name) if name in FIT else over_pair(name)


VIEW_CONFIGS = {n: (c[0], c[1], c[2], c[3]) for n, c in FIT.items()}
VIEW_CONFIGS.update({n: (c[0], c[1], c[2], (0, 0)) for n, c in OVER.items()})


class Ref:
    """A scene and what the CPU oracle makes of it: forward outputs, state and (grads=True) the gradients of upstream_grads
    -- with `zero` (a [B, H, W] boolean mask) the upstream gradients of those pixels zeroed."""

    def __init__(self, oracle, d, B, H, W, rows=(0, 0), grads=True, zero=None):
        self.d, self.B, self.H, self.W, self.rows = d, B, H, W, rows
        self.F = d["faces"].shape[0]
        self.sc = oracle.scene_from_module_inputs(d, H, W, rows=rows)
        self.color, self.depth, self.st = oracle.tri_forward(self.sc)
        self.gc, self.gd = upstream_grads(B, H, W)
        if zero is not None:
            keep = th.from_numpy(~zero).to(self.gc.dtype)[:, None]
            self.gc, self.gd = self.gc * keep, self.gd * keep
        self.grads = oracle.tri_backward(self.sc, self.st, self.gc.numpy(), self.gd.numpy()) if grads else None

    def band(self):
        """the pixel rows the call renders"""
        gy = (self.H + TILE - 1) // TILE
        r0, r1 = self.rows if self.rows != (0, 0) else (0, gy)
        return TILE * min(r0, gy), min(self.H, TILE * min(r1, gy))


def tile_pixels(mask, B, H, W):
    """per-tile booleans [B * gy * gx] -> per-pixel booleans [B, H, W]"""
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    m = np.asarray(mask, dtype=bool).reshape(B, gy, gx)
    return np.repeat(np.repeat(m, TILE, axis=1), TILE, axis=2)[:, :H, :W]


# ---- the classifier ----------------------------------------------------------------------------------------------------------
def _counts(st, ntiles):
    r = st.get("ranges").reshape(-1, 2).astype(np.int64)
    assert r.shape[0] == ntiles
    return r, r[:, 1] - r[:, 0]


def classify(stA, stB, B, F, H, W):
    """From the oracle's state of A (the placement's scene) and B (the scene binned into it) -> a dict:
    per tile `cA`, `cB`, `seg` (the segment's length) and `overflows`; `entries[route]`, the list entries of B per route, and
    `overflow_tiles[route]`, the overflowing tiles that receive entries through it; `big`, `max_big_per_workgroup`,
    `direct_big_faces` (big faces beyond their workgroup's queue); `fpt`, `straddles`; `sort` {path: busy tiles of B},
    `longest`, `chunks` (of MASK_CHUNK entries, the longest list's); `tiles`, `RA`, `RB`; `changed`, the tiles whose count
    differs; `gained_and_fits`; `neighbours`: busy tiles that keep their count and follow or precede an overflowing tile in
    tile order; `overflow_empty_in_A` / `overflow_busy_in_A`."""
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    T = gx * gy
    ntiles = B * T
    assert ntiles <= SCAN_SINGLE_MAX and T <= LDS_HIST_MAX, "not a frame the placed path takes"
    _, cA = _counts(stA, ntiles)
    rB, cB = _counts(stB, ntiles)
    seg = cA + cA // 4 + SEG_SLACK
    overflows = cB > seg
    # the route of every (view, face) pair of B
    BF = B * F
    fpt = bin_fpt(BF)
    per = 256 * fpt
    touched = stB.get("tiles_touched")
    assert touched.shape[0] == BF
    idx = np.arange(BF, dtype=np.int64)
    wg = idx // per
    mine = (idx // F) == ((wg * per) // F)
    big = touched > BIG_RECT
    nbig = np.bincount(wg[big], minlength=int(wg.max()) + 1 if BF else 1)
    route = np.where(big, np.where(nbig[wg] > BIG_MAX, 3, 1), np.where(mine, 0, 2))
    # ... and of every list entry
    values = stB.get("values").astype(np.int64)
    entry_tile = np.repeat(np.arange(ntiles, dtype=np.int64), cB)
    busy = cB > 0   # (the lists lie back to back in tile order; an empty tile's range is (0, 0))
    assert entry_tile.shape[0] == values.shape[0] and bool((rB[busy, 0] == (np.cumsum(cB) - cB)[busy]).all())
    entry_route = route[(entry_tile // T) * F + values]
    entries = {name: int((entry_route == k).sum()) for k, name in enumerate(ROUTES)}
    overflow_tiles = {name: int(np.unique(entry_tile[(entry_route == k) & overflows[entry_tile]]).shape[0]) for k, name in enumerate(ROUTES)}
    depth_bits = (stB.get("keys") & np.uint64(0xffffffff)).astype(np.uint32)
    sort = {"bucket": 0, "segmented": 0, "bitonic": 0}
    for t in np.nonzero(cB)[0]:
        sort[sort_path(depth_bits[rB[t, 0]:rB[t, 1]])] += 1
    first = np.arange(0, BF, per, dtype=np.int64)
    last = np.minimum(first + per, BF) - 1
    keeps = (cB == cA) & (cB > 0)
    nb = np.zeros(ntiles, dtype=bool)
    nb[1:] |= overflows[:-1]
    nb[:-1] |= overflows[1:]
    longest = int(cB.max()) if ntiles else 0
    return {
        "cA": cA, "cB": cB, "seg": seg, "overflows": overflows,
        "entries": entries, "overflow_tiles": overflow_tiles,
        "big": int(big.sum()), "max_big_per_workgroup": int(nbig.max()), "direct_big_faces": int(np.maximum(nbig - BIG_MAX, 0).sum()),
        "BF": BF, "fpt": fpt, "straddles": bool((first // F != last // F).any()),
        "sort": sort, "longest": longest, "chunks": -(-longest // MASK_CHUNK),
        "tiles": ntiles, "RA": int(cA.sum()), "RB": int(cB.sum()),
        "changed": int((cA != cB).sum()), "gained_and_fits": int(((cB > cA) & ~overflows).sum()),
        "neighbours": int((keeps & nb & ~overflows).sum()),
        "overflow_empty_in_A": int((overflows & (cA == 0)).sum()), "overflow_busy_in_A": int((overflows & (cA > 0)).sum()),
        "fill": float(cB.sum()) / float(seg.sum()),
    }


def summary(c):
    """classify()'s result without the per-tile arrays, for printing"""
    return {k: v for k, v in c.items() if not isinstance(v, np.ndarray)} | {"overflowing": int(c["overflows"].sum())}
