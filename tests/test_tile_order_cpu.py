"""The order placed calls take their tiles in (csrc/dmr_tile_order.hpp, used by build_placement in dmr_api.hip): blocks of
ORDER_BLOCK x ORDER_BLOCK tiles dealt heaviest first to 8 classes, class x owning the positions x, x + 8, ...; inside a class
busy tiles first, longest list first.  The header is plain C++; this compiles it with the host compiler into a small program
that reads cases from stdin and prints the orders, and checks the properties the rule promises -- first of all that the
output is a permutation (anything else would send a workgroup to a tile that does not exist)."""
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from dmesh_renderer_amd import scenes

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dmesh_renderer_amd", "csrc")
CLASSES = 8
# (the program below prints the constant too; the case list needs it before the program runs)
BLOCK = int(re.search(r"constexpr int ORDER_BLOCK = (\d+);", open(os.path.join(CSRC, "dmr_tile_order.hpp")).read()).group(1))

PROGRAM = r"""
#include <cstdio>
#include <vector>
#include "dmr_tile_order.hpp"
// stdin: cases "B gx gy has_pairs" + counts (+ pairs); stdout: "ORDER_BLOCK ORDER_CLASSES", then one line per case
int main() {
    printf("%d %d\n", dmr::ORDER_BLOCK, dmr::ORDER_CLASSES);
    int B, gx, gy, hp;
    while (scanf("%d %d %d %d", &B, &gx, &gy, &hp) == 4) {
        const size_t n = (size_t)B * gx * gy;
        std::vector<uint32_t> count(n), pairs(n), order(n, 0xffffffffu);
        for (auto& c : count) if (scanf("%u", &c) != 1) return 1;
        if (hp) for (auto& p : pairs) if (scanf("%u", &p) != 1) return 1;
        dmr::tile_order(B, gx, gy, count.data(), hp ? pairs.data() : nullptr, order.data());
        for (size_t i = 0; i < n; i++) printf("%u ", order[i]);
        printf("\n");
    }
    return 0;
}
"""


def c4_counts():
    """List entries per tile of C4 (1920 x 1080, 120 x 68 tiles), binned as k_project_verts / face_bin do it: float32
    operation by operation, the double division and pixel mapping of dmr_device.hpp."""
    cfg = scenes.CONFIGS["C4"]
    d = scenes.make("C4")
    H, W, f32 = cfg.H, cfg.W, np.float32
    gx, gy = (W + 15) // 16, (H + 15) // 16
    v = d["verts"].numpy().astype(f32)
    mv, pr = d["mv_mats"][0].numpy().astype(f32), d["proj_mats"][0].numpy().astype(f32)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    p = [mv[r, 0] * x + mv[r, 1] * y + mv[r, 2] * z + mv[r, 3] for r in range(3)]
    c = [pr[r, 0] * p[0] + pr[r, 1] * p[1] + pr[r, 2] * p[2] + pr[r, 3] for r in range(4)]
    w, eps = c[3].copy(), f32(1e-4)
    w[(w >= 0) & (w < eps)] = eps
    w[(w < 0) & (w > -eps)] = -eps
    pw = (1.0 / w.astype(np.float64)).astype(f32)
    px = ((((c[0] * pw).astype(np.float64) + 1.0) * W - 1.0) * 0.5).astype(f32)
    py = ((((c[1] * pw).astype(np.float64) + 1.0) * H - 1.0) * 0.5).astype(f32)
    pz = c[2] * pw
    f = d["faces"].numpy().astype(np.int64)
    X, Y, Z = px[f], py[f], pz[f]
    t = lambda a: np.trunc(a / f32(16)).astype(np.int64)
    minx, miny = np.clip(t(X.min(1)), 0, gx), np.clip(t(Y.min(1)), 0, gy)
    maxx, maxy = np.clip(t(X.max(1)) + 1, 0, gx), np.clip(t(Y.max(1)) + 1, 0, gy)
    seen = ~((Z.max(1) < -1.0) | (Z.min(1) > 1.0))
    count = np.zeros((gy + 1, gx + 1), dtype=np.int64)  # 2-D difference array of the rects
    for sx, sy, s in ((minx, miny, 1), (maxx, miny, -1), (minx, maxy, -1), (maxx, maxy, 1)):
        np.add.at(count, (sy[seen], sx[seen]), s)
    count = count.cumsum(0).cumsum(1)[:gy, :gx].reshape(-1)
    assert int(count.sum()) == 918402 and int((count > 0).sum()) == 2916  # the library's num_rendered, its busy tiles
    return gx, gy, count


def cases():
    rng = np.random.default_rng(7)
    half = lambda n: np.where(rng.random(n) < 0.5, rng.integers(1, 700, n), 0)
    gx4, gy4, c4 = c4_counts()
    out = [
        ("one tile", 1, 1, 1, np.array([5]), None),
        ("seven tiles", 1, 7, 1, np.array([3, 0, 9, 9, 1, 0, 4]), None),
        ("3 x 3", 1, 3, 3, np.array([0, 10, 20, 30, 0, 50, 60, 70, 80]), None),
        ("16 x 12, busy and empty", 1, 16, 12, half(192), None),
        ("16 x 12, with pairs", 1, 16, 12, half(192), rng.integers(0, 60000, 192)),
        ("all empty", 1, 16, 12, np.zeros(192, dtype=np.int64), None),
        ("all busy, equal counts", 1, 16, 12, np.full(192, 77), None),
        ("8 x 8, all busy", 1, 8, 8, rng.permutation(64) + 1, None),
        # ONE block, all of its tiles busy (ORDER_BLOCK 8: 64 tiles, 8 positions per class, 56 must spill)
        ("one full block", 1, BLOCK, BLOCK, rng.permutation(BLOCK * BLOCK) + 1, None),
        ("B = 2", 2, 11, 9, half(198), None),
        ("B = 2, first view empty", 2, 11, 9, np.concatenate([np.zeros(99, dtype=np.int64), half(99)]), None),
        ("C4", 1, gx4, gy4, c4, None),
    ]
    return out


@pytest.fixture(scope="module")
def orders():
    """-> (ORDER_BLOCK, [(name, B, gx, gy, count, pairs, order)]), one run of the compiled program for all cases."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    cs = cases()
    text = []
    for _, B, gx, gy, count, pairs in cs:
        text.append(f"{B} {gx} {gy} {int(pairs is not None)} " + " ".join(map(str, count))
                    + (" " + " ".join(map(str, pairs)) if pairs is not None else ""))
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "order.cpp"), os.path.join(tmp, "order")
        with open(src, "w") as f:
            f.write(PROGRAM)
        subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-I", CSRC, src, "-o", exe], check=True)
        res = subprocess.run([exe], input="\n".join(text) + "\n", capture_output=True, text=True, check=True)
    lines = res.stdout.strip().split("\n")
    block, classes = map(int, lines[0].split())
    assert classes == CLASSES and len(lines) == 1 + len(cs)
    return block, [c + (np.array(l.split(), dtype=np.int64),) for c, l in zip(cs, lines[1:])]


def block_ids(B, gx, gy, blk):
    t = np.arange(B * gx * gy)
    nbx, nby = (gx + blk - 1) // blk, (gy + blk - 1) // blk
    return ((t // (gx * gy)) * nby + (t // gx) % gy // blk) * nbx + t % gx // blk


def test_every_order_is_a_permutation(orders):
    for name, B, gx, gy, count, _, order in orders[1]:
        assert np.array_equal(np.sort(order), np.arange(B * gx * gy)), name


def test_busy_tiles_lead_each_class_longest_first(orders):
    for name, _, _, _, count, _, order in orders[1]:
        for x in range(CLASSES):
            c = count[order[x::CLASSES]]
            busy = c > 0
            assert not np.any(busy[1:] & ~busy[:-1]), (name, x, "a busy tile behind an empty one")
            assert np.all(np.diff(c[busy]) <= 0), (name, x, "busy counts must be non-increasing")


def test_a_blocks_tiles_share_a_class_unless_they_had_to_spill(orders):
    blk = orders[0]
    spills = {}
    for name, B, gx, gy, count, _, order in orders[1]:
        n = order.size
        cls = np.empty(n, dtype=np.int64)
        cls[order] = np.arange(n) % CLASSES
        block = block_ids(B, gx, gy, blk)
        spilled = 0
        for k in np.unique(block[count > 0]):
            ts = np.flatnonzero((block == k) & (count > 0))
            if np.unique(cls[ts]).size == 1:
                continue
            # they had to: some class of theirs -- the block's home -- has no position left (all of its positions hold busy
            # tiles) and whatever it kept is at least as long as every tile of the block that went elsewhere
            homes = []
            for h in np.unique(cls[ts]):
                kept = count[order[h::CLASSES]]
                away = ts[cls[ts] != h]
                if np.all(kept > 0) and count[away].max() <= kept.min():
                    homes.append(h)
            assert homes, (name, int(k), "tiles of one block in several classes without need")
            spilled += min(int((cls[ts] != h).sum()) for h in homes)
        spills[name] = spilled
    assert blk == BLOCK
    assert spills["one full block"] == blk * blk - (blk * blk + CLASSES - 1) // CLASSES  # all but class 0's positions
    assert spills["8 x 8, all busy"] == 64 - 8 * min(CLASSES, (8 // min(blk, 8)) ** 2)  # 8 positions per class that got a block
    assert spills["C4"] == 0
    assert spills["all empty"] == 0


def test_c4_classes_are_balanced_by_the_greedy_bound(orders):
    """Dealing heaviest first to the least loaded class: when the heaviest class received its last block it was the
    lightest, so it ends at most one block above the mean.  max <= mean + max block cost is the rule's own bound."""
    blk = orders[0]
    name, B, gx, gy, count, _, order = orders[1][-1]
    assert name == "C4"
    cost = np.where(count > 0, count + 44.0, 0.0)
    cls_cost = np.array([cost[order[x::CLASSES]].sum() for x in range(CLASSES)])
    block_cost = np.bincount(block_ids(B, gx, gy, blk), weights=cost)
    print("class costs", cls_cost, "max block", block_cost.max())
    assert cls_cost.max() <= cls_cost.mean() + block_cost.max()
