"""The tet renderer's edge scenes and the classifier that says which binning, sort and first-hit path each of them takes.

The tet renderer shares the tri renderer's front end (projection, face set-up, tile scan, scatter, per-tile sort) and adds the
first-hit kernel, which up to SCAN_SINGLE_MAX tiles sorts its own tile's list and above reads lists k_sort_tiles sorted.  CASES
are the scenes that reach what the parity scenes (a cube of side 2 seen from three units away) never do; classify() restates
the rules of dmr_sort.hpp, dmr_binning.hip and dmr_kernels.hpp on the CPU oracle's state, so tests/test_tet_paths_cpu.py can
assert without a GPU that every case reaches what it is for, and that the restated constants are still the kernels'.
tests/test_tet_paths_gpu.py runs the same scenes through the HIP path.
"""
import numpy as np
import torch as th

from dmesh_renderer_amd import scenes
from util import upstream_grads, with_bg

# ---- what the kernels decide by, restated (test_tet_paths_cpu.py checks each against the sources' text) ----------------------
SORT_LDS_KEYS = 2048      # dmr_sort.hpp: longer lists take the bitonic network in global memory
SORT_SMALL = 64           # dmr_sort.hpp: lists up to here skip the buckets (segmented rank sort)
SORT_NB_LOG2 = 6          # dmr_sort.hpp: 64 order-preserving buckets
SORT_BUCKET_MAX = 96      # dmr_sort.hpp: a fuller bucket sends the tile to the segmented rank sort
FI_CHUNK = 256            # dmr_tet.hip: list entries the first-hit walk stages at a time
BIG_RECT = 256            # dmr_binning.hip: a face whose rect covers more tiles is emitted by the whole workgroup
BIG_MAX = 128             # dmr_binning.hip: ... while its workgroup's queue has room
SCAN_SINGLE_MAX = 8192    # dmr_kernels.hpp: up to here one workgroup scans, and the first-hit kernel sorts its own tile
FPT_2, FPT_4 = 256 * 1024, 1024 * 1024   # dmr_binning.hip, bin_fpt: (view, face) pairs from which a thread takes 2 / 4 faces
TILE = 16


def bin_fpt(n):
    return 1 if n < FPT_2 else 2 if n < FPT_4 else 4


def padded(n):
    """dmr_api.hip: the capacity guessed from an estimate of n entries."""
    return n + n // 4 + 4096


# ---- the scenes --------------------------------------------------------------------------------------------------------------
OPACITY = (0.01, 0.1)   # low on purpose: the march's T threshold is reached rarely, topology does not hinge on expf ulps
W_MARGIN = 1e-3         # no vertex of a scaled scene lies this close to a view's plane w = 0

CASES = {
    # name: (m, B, H, W, scale)
    "tiles_8192": (3, 1, 1024, 2048, 1.0),      # exactly SCAN_SINGLE_MAX tiles: the last frame whose first-hit kernel sorts, slab full
    "tiles_8320": (3, 1, 1040, 2048, 1.0),      # k_tet_first_intersect<false>, k_sort_tiles, three-launch scan
    "tiles_two_views": (3, 2, 1040, 1040, 1.0),  # above 8 192 tiles only because of the second view (second scan block)
    "mixed_sorts": (6, 1, 64, 64, 1.0),         # bucket and segmented tiles in one frame, lists longer than FI_CHUNK
    "long_lists": (8, 1, 48, 48, 1.0),          # segmented and bitonic in one frame
    "all_bitonic": (12, 1, 32, 32, 1.0),        # every tile bitonic, >= 25 chunks per first-hit walk
    "inside_m4": (4, 2, 320, 320, 4.0),         # camera inside the mesh; more big faces in one workgroup than BIG_MAX
    "inside_m7": (7, 2, 320, 320, 4.0),         # the same with long lists everywhere
    "fpt2": (20, 3, 48, 64, 1.0),               # two faces per thread, workgroups straddle views
    "fpt4": (20, 11, 32, 48, 1.0),              # four faces per thread
}
ROWS_CASE, ROWS = "tiles_8320", (9, 41)         # ... and once as a band of tile rows
INSIDE = ("inside_m4", "inside_m7")             # ... and once more over a background
SORT_CASES = ("mixed_sorts", "long_lists", "all_bitonic")

# the pair of scenes whose second refutes the size guess the first leaves (same shapes: same size key and B * F bucket)
REDO = dict(m=10, B=1, H=160, W=176, seed=3, opacity=(0.02, 0.3), scales=(0.2, 1.0, 0.2, 1.0))


def kuhn(m, B, H, W, scale=1.0, seed=0, opacity=OPACITY):
    """scenes.kuhn_tets with verts *= scale.  A scaled scene's verts_depth -- an input attribute only -- is seeded noise: the
    true NDC z of a vertex near the eye plane is enormous, and an absolute bar on the depth image would mean nothing."""
    d = scenes.kuhn_tets(m, B, H, W, seed=seed, opacity=opacity)
    if scale != 1.0:
        d["verts"] = d["verts"] * scale
        P = d["verts"].shape[0]
        d["verts_depth"] = th.randn(B, P, generator=th.Generator().manual_seed(1000 + seed))
        vh = th.cat([d["verts"].double(), th.ones(P, 1, dtype=th.float64)], dim=1)
        w = th.einsum("bij,pj->bpi", d["proj_mats"].double() @ d["mv_mats"].double(), vh)[..., 3]
        assert float(w.abs().min()) > W_MARGIN, "a vertex on a view's plane w = 0"
    assert bool(th.isfinite(d["verts_depth"]).all())
    return d


def make(name):
    m, B, H, W, scale = CASES[name]
    return kuhn(m, B, H, W, scale), B, H, W


def redo_scene(scale):
    r = REDO
    return kuhn(r["m"], r["B"], r["H"], r["W"], scale, seed=r["seed"], opacity=r["opacity"])


class Ref:
    """A scene and what the CPU oracle makes of it: forward outputs, state and (grads=True) the gradients of upstream_grads."""

    def __init__(self, oracle, d, B, H, W, rows=(0, 0), grads=True):
        self.d, self.B, self.H, self.W, self.rows = d, B, H, W, rows
        self.F = d["faces"].shape[0]
        self.sc = oracle.scene_from_module_inputs(d, H, W, rows=rows)
        self.color, self.depth, self.active, self.st = oracle.tet_forward(self.sc)
        self.gc, self.gd = upstream_grads(B, H, W)
        self.grads = oracle.tet_backward(self.sc, self.st, self.gc.numpy(), self.gd.numpy()) if grads else None

    def band(self):
        """the pixel rows the call renders"""
        gy = (self.H + TILE - 1) // TILE
        r0, r1 = self.rows if self.rows != (0, 0) else (0, gy)
        return TILE * min(r0, gy), min(self.H, TILE * min(r1, gy))

    def classify(self):
        return classify(self.st, self.B, self.F, self.H, self.W)


def reference(oracle, name, rows=(0, 0), bg=False, grads=True):
    d, B, H, W = make(name)
    return Ref(oracle, with_bg(d) if bg else d, B, H, W, rows, grads)


# ---- the classifier ----------------------------------------------------------------------------------------------------------
def sort_path(depth_bits):
    """Which branch of sort_tile (dmr_sort.hpp) a list with these depth keys takes: lists beyond SORT_LDS_KEYS the bitonic
    network; up to 64 entries, or with more than SORT_BUCKET_MAX keys in one bucket, the segmented rank sort; else the buckets,
    bucket = (depth bits - the tile's minimum) >> max(bit length of the range - SORT_NB_LOG2, 0)."""
    n = depth_bits.shape[0]
    if n > SORT_LDS_KEYS:
        return "bitonic"
    if n <= SORT_SMALL:
        return "segmented"
    d = depth_bits.astype(np.int64)
    mn = int(d.min())
    shift = max(int(d.max() - mn).bit_length() - SORT_NB_LOG2, 0)
    return "segmented" if int(np.bincount((d - mn) >> shift).max()) > SORT_BUCKET_MAX else "bucket"


def classify(st, B, F, H, W):
    """From the oracle's state: tiles, R, the busy tiles (and those numbered SCAN_SINGLE_MAX and up: the later scan blocks'), the
    longest list (and its chunks of FI_CHUNK), the tiles on each sort path (`small`:
    those of `segmented` with at most 64 entries; `ties`: per path, the tiles that hold a duplicated depth key -- sorted by face
    id there), the (view, face) pairs with tiles_touched > BIG_RECT, the most of those in one set-up workgroup (256 * FPT
    consecutive pairs), FPT, and whether a workgroup holds pairs of two views."""
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    tiles = B * gx * gy
    ranges = st.get("ranges").reshape(-1, 2).astype(np.int64)
    assert ranges.shape[0] == tiles
    depth_bits = (st.get("keys") & np.uint64(0xffffffff)).astype(np.uint32)
    lens = ranges[:, 1] - ranges[:, 0]
    paths = {"bucket": 0, "segmented": 0, "bitonic": 0}
    ties = dict(paths)
    small = 0
    for t in np.nonzero(lens)[0]:
        k = depth_bits[ranges[t, 0]:ranges[t, 1]]
        p = sort_path(k)
        paths[p] += 1
        small += int(k.shape[0] <= SORT_SMALL)
        ties[p] += int((k[1:] == k[:-1]).any())   # (the oracle's keys are sorted)
    BF = B * F
    fpt = bin_fpt(BF)
    per = 256 * fpt
    big = np.nonzero(st.get("tiles_touched") > BIG_RECT)[0]
    first = np.arange(0, BF, per, dtype=np.int64)
    last = np.minimum(first + per, BF) - 1
    return {
        "tiles": tiles, "R": st.num_rendered, "busy": int((lens > 0).sum()), "longest": int(lens.max()) if tiles else 0,
        "busy_beyond_first_scan_block": int((lens[SCAN_SINGLE_MAX:] > 0).sum()),
        "chunks": int(-(-int(lens.max()) // FI_CHUNK)) if tiles else 0,
        "bucket": paths["bucket"], "segmented": paths["segmented"], "bitonic": paths["bitonic"], "small": small, "ties": ties,
        "big": int(big.shape[0]), "max_big_per_workgroup": int(np.bincount(big // per).max()) if big.shape[0] else 0,
        "BF": BF, "fpt": fpt, "straddles": bool((first // F != last // F).any()),
    }
