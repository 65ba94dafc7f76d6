// dmr_shade_table.hpp -- what the backward kernels of the shading units (dmr_shade.hip, dmr_texture.hip) share: the merge of
// a wave's lanes of equal key, and the per-tile LDS table their sums go through before they leave the CU.
#pragma once

#include <cstdint>

#include <hip/hip_runtime.h>

namespace dmr {

// The per-tile table (the scheme of k_tri_backward_hits' vertex table, dmr_tri.hip, in a copy the shading kernels own):
// STAB slots, open addressing, at most STAB_PROBES probes, then the row goes out with direct atomics.
constexpr int STAB = 560;
constexpr int STAB_PROBES = 16;
constexpr uint32_t STAB_EMPTY = 0xffffffffu;

// ---------------------------------------------------------------------------
// Lanes that hold the same key (a face) merge before they go to the table: four butterfly levels inside a 16-lane DPP row
// (lane ^ 1, ^ 2 by quad_perm, + 4, + 8 by row shifts), as k_tet_fragment_grads does: at every level a live lane whose partner
// is alive with the same key takes the partner's values and the partner retires.  Values move with selects, so a non-finite
// value stays with its own key.
// ---------------------------------------------------------------------------
template <int LEVEL, int NV>
__device__ __forceinline__ void shade_merge_level(int lane, int& key, float (&g)[NV]) {
    constexpr int offset = 1 << LEVEL;
    constexpr int FROM_UPPER = LEVEL == 0 ? 0xB1 : (LEVEL == 1 ? 0x4E : (LEVEL == 2 ? 0x104 : 0x108));  // quad_perm ^1, ^2; row_shl:4, :8
    constexpr int FROM_LOWER = LEVEL == 0 ? 0xB1 : (LEVEL == 1 ? 0x4E : (LEVEL == 2 ? 0x114 : 0x118));  // ... row_shr:4, :8
    const bool lower = (lane & offset) == 0;
    const int k_up = __builtin_amdgcn_update_dpp(-1, key, FROM_UPPER, 0xF, 0xF, false);  // key of lane + offset (as seen by lower lanes)
    const int k_lo = __builtin_amdgcn_update_dpp(-1, key, FROM_LOWER, 0xF, 0xF, false);  // key of lane - offset (as seen by upper lanes)
    const bool take = lower && key >= 0 && k_up == key;
    const bool retire = !lower && key >= 0 && k_lo == key;
#pragma unroll
    for (int c = 0; c < NV; c++) {
        const float other = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(g[c]), FROM_UPPER, 0xF, 0xF, false));
        g[c] += take ? other : 0.f;
    }
    if (retire) key = -1;
}
template <int NV>
__device__ __forceinline__ void shade_merge(int lane, int& key, float (&g)[NV]) {
    shade_merge_level<0>(lane, key, g);
    shade_merge_level<1>(lane, key, g);
    shade_merge_level<2>(lane, key, g);
    shade_merge_level<3>(lane, key, g);
}

// the slot of row `rid` in a table of N slots; -1: none within STAB_PROBES probes (the row goes out with direct atomics)
template <int N>
__device__ __forceinline__ int stab_find_n(uint32_t* __restrict__ key, uint32_t rid) {
    uint32_t s = __umulhi(rid * 2654435761u, (uint32_t)N);
    for (int i = 0; i < STAB_PROBES; i++) {
        const uint32_t prev = atomicCAS(&key[s], STAB_EMPTY, rid);
        if (prev == STAB_EMPTY || prev == rid) return (int)s;
        s = s + 1u == (uint32_t)N ? 0u : s + 1u;
    }
    return -1;
}
__device__ __forceinline__ int stab_find(uint32_t* __restrict__ key, uint32_t rid) { return stab_find_n<STAB>(key, rid); }

}  // namespace dmr
