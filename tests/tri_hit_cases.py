"""The tri renderer's edge scenes for the opt-in variants of k_tri_backward_hits (TRI_GRAD_EXACT, TRI_GRAD_CAMERA) and the
classifier that says which of the kernel's hard paths each of them reaches.

grad_cases.TRI_CASES -- three layers of 8 x 8 or 9 x 9 lattices in frames of at most 60 tiles -- give a tile a few dozen vertex
rows and a few hundred records, stop no pixel early and hold no face of opacity 1.  CASES are the scenes that reach what those
never do; classify() restates the rules of dmr_tri.hip and dmr_kernels.hpp on the CPU oracle's state and the float64 model's
pair lists, so tests/test_tri_hit_paths_cpu.py can assert without a GPU that every case reaches what it is for, and that the
restated constants are still the kernels'.  tests/test_tri_hit_paths_gpu.py runs the same scenes through the HIP path.

Long lists come from STACKED COPIES, not from dense scenes.  The float64 model (tests/tri_grad_ref.py) drops every pixel whose
centre lies within EDGE_EPS of an edge of a listed face; with many independently jittered layers of small faces nearly every
pixel does (layered_sheets(12, 9, ...), (40, 9, ...) and (14, 6, ...) keep 40-72 % of the pixels, of which 100-600 hold
pairs).  So the faces of a long list must have coinciding projected edges: stacked(d, c) repeats a small scene's vertices c
times at the same positions under distinct vertex ids, and face copy i indexes vertex copy i.  The model keeps as many pixels
as for the base scene, a tile's list is c times as long and holds c times as many distinct vertex rows.
"""
import numpy as np
import torch as th

import grad_cases
from dmesh_renderer_amd import scenes
from tri_grad_ref import T_EPS, TriGradRef
from util import upstream_grads

# ---- what the kernels decide by, restated (test_tri_hit_paths_cpu.py checks each against the sources' text) ------------------
VTAB = 560              # dmr_tri.hip: vertex-row slots of a workgroup's table
TAB_PROBES = 16         # dmr_tri.hip: probes before tab_find3 gives up (-1: the row leaves through direct atomics)
HIT_GROUP = 4           # dmr_kernels.hpp: records of one lane; a face's run in a tile is padded to a multiple
ROUND_GROUPS = 256      # dmr_tri.hip, k_tri_backward_hits: one group per thread and round (for g0 ... += 256u)
ROUND_RECORDS = ROUND_GROUPS * HIT_GROUP
TILE = 16
REDUCE_THREADS = 1024   # k_tri_camera_reduce's workgroup
TRI_N, TET_N = 32, 64   # floats per tile partial: dmr_api.hip's two launch_camera_reduce calls
assert T_EPS == 1e-4    # dmr_device.hpp (tri_grad_ref restates it)


def reduce_rows(N):
    """k_tri_camera_reduce<N>: Q = N / 4 float4 per partial, ROWS = 1024 / Q thread rows."""
    return REDUCE_THREADS // (N // 4)


def reduce_unrolled_from(N):
    """Tiles per view from which some thread row runs the four-loads-in-flight loop (t + 3 * ROWS < tiles at t = 0)."""
    return 3 * reduce_rows(N) + 1


def reduce_unrolled_all(N):
    """... from which every thread row does (t = ROWS - 1): more than 4 * ROWS - 1 tiles."""
    return 4 * reduce_rows(N)


# ---- the scenes --------------------------------------------------------------------------------------------------------------
def stacked(d, c):
    """c copies of the scene d in one: the vertices repeated at the same positions under distinct ids with fresh seeded colours,
    face copy i on vertex copy i (opacity and intensity drawn per copy from the base scene's own values, permuted)."""
    P, F = d["verts"].shape[0], d["faces"].shape[0]
    g = th.Generator().manual_seed(4000 + c)
    perm = th.stack([th.randperm(F, generator=g) for _ in range(c)])                      # [c, F]
    return dict(
        d,
        verts=d["verts"].repeat(c, 1),
        faces=th.cat([d["faces"] + i * P for i in range(c)], 0).to(th.int32),
        verts_color=th.rand(c * P, 3, generator=g, dtype=th.float64).to(th.float32),
        faces_opacity=d["faces_opacity"][perm].reshape(-1),
        faces_intense=th.cat([d["faces_intense"][:, perm[i]] for i in range(c)], 1).contiguous(),
        verts_depth=d["verts_depth"].repeat(1, c),
    )


CROWDED_OPACITY = (0.002, 0.01)   # 300 faces deep and T still above 0.04: no pixel of a crowded case stops early
CASES = {
    # name: (L, n, B, H, W, seed, opacity, copies, every how many faces one of opacity 1)
    "crowded_one_tile": (2, 3, 1, 16, 16, 5, CROWDED_OPACITY, 150, 0),    # one workgroup, >= 27 rounds, 2 700 rows for 560 slots
    "crowded_four_tiles": (3, 4, 1, 32, 32, 5, CROWDED_OPACITY, 70, 0),
    "crowded_two_views": (3, 4, 2, 32, 48, 5, CROWDED_OPACITY, 40, 0),
    "opaque_deep": (14, 3, 1, 96, 144, 3, (0.45, 0.9), 1, 11),            # early stops, T == 0 behind faces of opacity 1, huge faces
    "opaque_two_views": (14, 3, 2, 48, 80, 3, (0.45, 0.9), 1, 11),
    "wide": (3, 9, 1, 353, 361, 7, (0.1, 0.5), 1, 0),                     # 23 x 23 tiles, the last row one pixel high, the last column nine wide
    "wide_two_views": (2, 6, 2, 353, 361, 7, (0.1, 0.5), 1, 0),
}
CROWDED = tuple(k for k in CASES if k.startswith("crowded"))
OPAQUE = tuple(k for k in CASES if k.startswith("opaque"))
WIDE = tuple(k for k in CASES if k.startswith("wide"))

TET_WIDE = {
    # name: (m, B, H, W, opacity, ray_random_seed): 17 x 17 tiles per view, the last row one pixel high, the last column nine wide
    "tet_wide": (4, 1, 257, 265, (0.02, 0.3), 0),
    "tet_wide_two_views": (3, 2, 257, 265, (0.05, 0.5), 0),
}


def make(name):
    L, n, B, H, W, seed, opacity, copies, opaque_every = CASES[name]
    d = scenes.layered_sheets(L, n, B, H, W, seed=seed, opacity=opacity)
    if opaque_every:
        d["faces_opacity"][::opaque_every] = 1.0
    if copies > 1:
        d = stacked(d, copies)
    return d, B, H, W


def tet_scene(name):
    m, B, H, W, op, seed = TET_WIDE[name]
    return scenes.kuhn_tets(m, B, H, W, seed=0, opacity=op), B, H, W, seed


_tet_refs = {}


def tet_reference(oracle, name):
    """(d, B, H, W, seed) of a TET_WIDE scene and grad_cases.reference's (TetCameraGradRef, masked upstream, its gradients),
    once per case and module."""
    if name not in _tet_refs:
        sc = tet_scene(name)
        _tet_refs[name] = sc + grad_cases.reference(oracle, *sc, camera=True)
    return _tet_refs[name]


# ---- the reference, once per case and module ---------------------------------------------------------------------------------
GRAD_KEYS = ("verts", "verts_color", "faces_opacity", "verts_depth", "faces_intense")
EXACT_KEYS = GRAD_KEYS[1:]   # what the reference renderer differentiates exactly: the oracle and the model must agree on these


class Ref:
    """A scene, what the CPU oracle makes of it, the float64 model, the upstream gradients masked to the pixels the model keeps
    and scaled by `factor`, and the model's gradients of that upstream.

    factor: the gradients are linear in the upstream, and rel_err's max(1, .) makes the bar an absolute one where the
    reference stays below 1 (the crowded cases: faces of opacity <= 0.01).  So both masked upstream tensors are multiplied by one
    power of two, the smallest that lifts the largest entry of each of the model's seven gradients to 1 -- chosen from the model
    alone, exact on both sides."""

    def __init__(self, oracle, d, B, H, W):
        self.d, self.B, self.H, self.W = d, B, H, W
        self.sc = oracle.scene_from_module_inputs(d, H, W)
        self.color, self.depth, self.st = oracle.tri_forward(self.sc)
        self.model = TriGradRef(d, H, W, self.st)
        gc, gd = upstream_grads(B, H, W)
        m = self.model.mask()
        gc, gd = gc * m, gd * m
        g1, self.model_color, self.model_depth = self.model.grads(gc, gd)
        smallest = min(float(np.abs(v).max()) for v in g1.values())
        assert smallest > 0
        self.factor = 2.0 ** max(0, int(np.ceil(-np.log2(smallest))))
        self.gc, self.gd = gc * self.factor, gd * self.factor
        self.grads = {k: v * self.factor for k, v in g1.items()}
        self._oracle_grads = None

    def oracle_grads(self, oracle):
        if self._oracle_grads is None:
            self._oracle_grads = oracle.tri_backward(self.sc, self.st, self.gc.numpy(), self.gd.numpy())
        return self._oracle_grads

    def classify(self):
        return classify(self.st, self.model, self.d, self.B, self.H, self.W)


_refs = {}


def reference(oracle, name):
    if name not in _refs:
        _refs[name] = Ref(oracle, *make(name))
    return _refs[name]


# ---- the classifier ----------------------------------------------------------------------------------------------------------
def classify(st, model, d, B, H, W):
    """From the oracle's state and the model's pair lists.  Per tile (arrays over B * gy * gx tiles): `list` the list length;
    `rows` the distinct vertex rows of its list; `rows_blended` those of the faces the kept pixels blend (what k_tri_backward_hits
    looks up in its table, at least); `records` a lower bound on the tile's records -- the kept pixels' pairs per face, each
    face's run padded to HIT_GROUP (the dropped pixels' pairs come on top); `rounds` the rounds of ROUND_RECORDS that implies.
    Per case: the kept pixels that end at T == 0 and at 0 < T < T_EPS (the oracle's final_T), the tiles per view, the kept
    fraction, the model's pairs and its longest pixel list."""
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    tiles = B * gx * gy
    ranges = st.get("ranges").reshape(-1, 2).astype(np.int64)
    assert ranges.shape[0] == tiles
    values = st.get("values").astype(np.int64)
    faces = d["faces"].numpy().astype(np.int64)
    F = faces.shape[0]
    rows = np.zeros(tiles, np.int64)
    for t in np.nonzero(ranges[:, 1] > ranges[:, 0])[0]:
        rows[t] = np.unique(faces[values[ranges[t, 0]:ranges[t, 1]]]).shape[0]
    # the model's pairs (pixel, face) -> per (tile, face) counts
    fo = model.faces_of.numpy()
    live = fo >= 0
    tile_of = (model.view.numpy() * gy + model.py.numpy() // TILE) * gx + model.px.numpy() // TILE
    key = (tile_of[:, None] * F + fo)[live]
    uniq, cnt = np.unique(key, return_counts=True)
    ut, uf = uniq // F, uniq % F
    padded = (cnt + HIT_GROUP - 1) // HIT_GROUP * HIT_GROUP
    records = np.bincount(ut, weights=padded, minlength=tiles).astype(np.int64)
    rows_blended = np.zeros(tiles, np.int64)
    for t in np.unique(ut):
        rows_blended[t] = np.unique(faces[uf[ut == t]]).shape[0]
    final_T = st.get("final_T").reshape(B, H, W)
    kept = model.keep.numpy()
    return {
        "tiles": tiles, "tiles_per_view": gx * gy, "kept": model.kept_fraction,
        "list": ranges[:, 1] - ranges[:, 0], "rows": rows, "rows_blended": rows_blended, "records": records,
        "rounds": (records + ROUND_RECORDS - 1) // ROUND_RECORDS,
        "T_zero": int((kept & (final_T == 0)).sum()), "T_below_eps": int((kept & (final_T > 0) & (final_T < T_EPS)).sum()),
        "pairs": int(live.sum()), "K": int(fo.shape[1]),
    }


def summary(c):
    """classify()'s result with the per-tile arrays replaced by their largest entries (for printing)."""
    return {k: (int(v.max()) if isinstance(v, np.ndarray) else v) for k, v in c.items()}
