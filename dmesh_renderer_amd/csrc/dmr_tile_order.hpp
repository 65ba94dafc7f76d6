// dmr_tile_order.hpp -- the order in which the compositing kernels of a PLACED call take their tiles (dmr_api.hip,
// build_placement).  Plain C++, no HIP: the CPU tests compile it on its own (tests/test_tile_order_cpu.py).
//
// Workgroups of a 1-D grid are dealt round-robin over the 8 XCDs of the chip, each with an L2 of its own (observed:
// scripts/micro/xcc_probe.hip; nothing here is needed for correctness -- ANY permutation renders the same image).  With
// "longest list first" over the whole frame the tiles one XCD composites are a random eighth of the image, and its L2
// sees nearly the whole mesh.  Here neighbouring tiles stay on one XCD:
//   * tiles are grouped into blocks of ORDER_BLOCK x ORDER_BLOCK tiles per view (partial blocks at the right and bottom edges);
//   * a block costs the sum over its busy tiles of  entries + 44 + 0.083 * blended pairs  (DESIGN.md section 7's fitted
//     model in entry units; without pairs: entries + 44);
//   * blocks are dealt heaviest first to the class (of ORDER_CLASSES) with the smallest load so far;
//   * class x owns the positions x, x + 8, x + 16, ...: its busy tiles take the first of them by non-increasing entry
//     count (longest first INSIDE a class: the longest chain still starts first), empty tiles fill what is left;
//   * a class with more busy tiles than positions spills its shortest ones into free positions of other classes
//     (correct anywhere; only their locality is lost).
// pos % 8 and (pos + 1) % 8 split the positions into the same classes, so one order serves the forward, whose tile at
// position pos is workgroup pos + 1, and the backward kernels.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

namespace dmr {

constexpr int ORDER_BLOCK = 4;    // tiles per block edge (2 .. 16 measured at C4 and C2: profiles/tile_order/block_size.txt)
constexpr int ORDER_CLASSES = 8;  // XCDs

// count[t]: list entries of tile t (t = (view * gy + ty) * gx + tx, 0: empty -- every tile outside a shard's band);
// pairs[t]: its blended (pixel, face) pairs, or null.  order[0 .. B * gx * gy): the permutation.
inline void tile_order(int B, int gx, int gy, const uint32_t* count, const uint32_t* pairs, uint32_t* order, int block = ORDER_BLOCK) {
    const int ntiles = B * gx * gy;
    const int nclass = std::min(ORDER_CLASSES, ntiles);  // (classes that own a position)
    if (ntiles <= 0) return;
    const int nbx = (gx + block - 1) / block, nby = (gy + block - 1) / block, nblocks = B * nbx * nby;
    auto block_of = [&](int t) { return ((t / (gx * gy)) * nby + (t / gx) % gy / block) * nbx + t % gx / block; };
    auto room = [&](int x) { return (ntiles - x + ORDER_CLASSES - 1) / ORDER_CLASSES; };  // positions of class x

    std::vector<double> cost((size_t)nblocks, 0.0);
    for (int t = 0; t < ntiles; t++)
        if (count[t]) cost[(size_t)block_of(t)] += (double)count[t] + 44.0 + (pairs ? 0.083 * (double)pairs[t] : 0.0);
    std::vector<int> heavy;  // the blocks with busy tiles, heaviest first
    for (int k = 0; k < nblocks; k++) if (cost[(size_t)k] > 0.0) heavy.push_back(k);
    std::stable_sort(heavy.begin(), heavy.end(), [&](int a, int b) { return cost[(size_t)a] > cost[(size_t)b]; });
    std::vector<int> home((size_t)nblocks, 0);
    double load[ORDER_CLASSES] = {};
    for (int k : heavy) {
        int x = 0;
        for (int y = 1; y < nclass; y++) if (load[y] < load[x]) x = y;
        home[(size_t)k] = x; load[x] += cost[(size_t)k];
    }

    auto longer = [&](uint32_t a, uint32_t b) { return count[a] > count[b]; };
    std::vector<uint32_t> busy[ORDER_CLASSES], spilled, empty;
    for (int t = 0; t < ntiles; t++) {
        if (count[t]) busy[home[(size_t)block_of(t)]].push_back((uint32_t)t);
        else empty.push_back((uint32_t)t);
    }
    for (int x = 0; x < nclass; x++) {
        std::stable_sort(busy[x].begin(), busy[x].end(), longer);
        const size_t keep = (size_t)room(x);
        if (busy[x].size() > keep) {  // the shortest ones leave
            spilled.insert(spilled.end(), busy[x].begin() + (std::ptrdiff_t)keep, busy[x].end());
            busy[x].resize(keep);
        }
    }
    if (!spilled.empty()) {  // each into the class with the most free positions (busy tiles <= tiles: there is one)
        std::stable_sort(spilled.begin(), spilled.end(), longer);
        for (uint32_t t : spilled) {
            int x = -1; size_t most = 0;
            for (int y = 0; y < nclass; y++) {
                const size_t left = (size_t)room(y) - busy[y].size();
                if (left > most) { most = left; x = y; }
            }
            busy[x].push_back(t);
        }
        for (int x = 0; x < nclass; x++) std::stable_sort(busy[x].begin(), busy[x].end(), longer);
    }
    size_t e = 0;
    for (int x = 0; x < nclass; x++) {
        const size_t n = (size_t)room(x);
        for (size_t k = 0; k < n; k++) order[(size_t)x + ORDER_CLASSES * k] = k < busy[x].size() ? busy[x][k] : empty[e++];
    }
}

}  // namespace dmr
