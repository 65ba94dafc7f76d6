// dmr_shade_common.hpp -- what the shading units over fragment lists (dmr_shade.hip, dmr_texture.hip, dmr_visibility.hip,
// dmr_interp.hip, dmr_packed.hip; the last three through dmr_deferred_common.hpp, which adds what they alone share) share, each
// fact once:
//   device: the merge of a wave's lanes of equal key (shade_merge; shade_merge_max for a maximum) and the per-tile LDS table
//           (stab_find*).  The kernels' walks are each unit's own text, those they have in common too: DESIGN.md 5c;
//   host:   the list arguments' validation (shade_check_sizes, shade_check_lists), shade_vec, the K ladder (with_kmax), the
//           backward calls' prologue (shade_backward_prologue), the check after a launch (launched).
#pragma once

#include <cstdint>
#include <initializer_list>
#include <string>
#include <type_traits>

#include <hip/hip_runtime.h>

#include "dmr_kernels.hpp"

namespace dmr {

int api_fail(const char* m);  // dmr_api.hip: sets dmr_last_error()'s message, returns 1

// The per-tile table (the scheme of k_tri_backward_hits' vertex table, dmr_tri.hip, in a copy the shading kernels own):
// STAB slots, open addressing, at most STAB_PROBES probes, then the row goes out with direct atomics.
constexpr int STAB = 560;
constexpr int STAB_PROBES = 16;
constexpr uint32_t STAB_EMPTY = 0xffffffffu;

// ---------------------------------------------------------------------------
// Lanes that hold the same key (a face) merge before they go to the table: four butterfly levels inside a 16-lane
// DPP row (lane ^ 1, ^ 2 by quad_perm, + 4, + 8 by row shifts), as k_tet_fragment_grads does: at every level a live lane whose
// partner is alive with the same key takes the partner's values and the partner retires.  Values move with selects, so a
// non-finite value stays with its own key.
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

// The same merge for a value that is a maximum, not a sum (dmr_visibility.hip's largest weight): run it on a COPY of the key
// shade_merge is about to get -- the keys alone decide who takes and who retires, so both end on the same survivors.
template <int LEVEL>
__device__ __forceinline__ void shade_merge_max_level(int lane, int& key, float& m) {
    constexpr int offset = 1 << LEVEL;
    constexpr int FROM_UPPER = LEVEL == 0 ? 0xB1 : (LEVEL == 1 ? 0x4E : (LEVEL == 2 ? 0x104 : 0x108));
    constexpr int FROM_LOWER = LEVEL == 0 ? 0xB1 : (LEVEL == 1 ? 0x4E : (LEVEL == 2 ? 0x114 : 0x118));
    const bool lower = (lane & offset) == 0;
    const int k_up = __builtin_amdgcn_update_dpp(-1, key, FROM_UPPER, 0xF, 0xF, false);
    const int k_lo = __builtin_amdgcn_update_dpp(-1, key, FROM_LOWER, 0xF, 0xF, false);
    const bool take = lower && key >= 0 && k_up == key;
    const bool retire = !lower && key >= 0 && k_lo == key;
    const float other = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(m), FROM_UPPER, 0xF, 0xF, false));
    m = (take && other > m) ? other : m;
    if (retire) key = -1;
}
__device__ __forceinline__ void shade_merge_max(int lane, int key, float& m) {
    shade_merge_max_level<0>(lane, key, m);
    shade_merge_max_level<1>(lane, key, m);
    shade_merge_max_level<2>(lane, key, m);
    shade_merge_max_level<3>(lane, key, m);
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

// ---- Host side of the C calls.  A refusal returns non-zero with dmr_last_error()'s message set; `n` is the call's name and
// ": ".  The first check that fails decides the message: a unit calls shade_check_sizes, its own size checks, shade_check_lists.
inline int shade_check_sizes(const std::string& n, int B, int K, int H, int W, int P, int F, int C, int max_c) {
    if (B <= 0 || H <= 0 || W <= 0 || P < 0 || F < 0) return api_fail((n + "bad dimensions").c_str());
    if (K < 1 || K > FRAG_MAX_K) return api_fail((n + "K must be in 1.." + std::to_string(FRAG_MAX_K) + ", got " + std::to_string(K)).c_str());
    if (C < 1 || C > max_c) return api_fail((n + "C must be in 1.." + std::to_string(max_c) + ", got " + std::to_string(C)).c_str());
    return 0;
}

// The pointers and the grid -> the list fields of the unit's parameter block l, which both blocks spell under the same names
// (a struct of them inside the blocks moves the other fields, and with that the kernels' SGPR spills and rounding: DESIGN.md 5c).
// corner_name: "faces" / "uv_faces"; missing: the first of the unit's own tensors that is null though needed, or null.
template <class P>
int shade_check_lists(const std::string& n, const char* corner_name, int B, int K, int H, int W, int F, const int32_t* face,
                             const float* bary, const int32_t* corners, const float* faces_opacity, const float* face_scale,
                             const char* missing, P& l) {
    if (!face || !bary) return api_fail((n + "null fragment lists").c_str());
    if (F > 0 && (!corners || !faces_opacity)) return api_fail((n + "null " + corner_name + " / faces_opacity").c_str());
    if (missing) return api_fail((n + "null " + missing).c_str());
    const int64_t gx = (W + TILE - 1) / TILE, gy = (H + TILE - 1) / TILE;
    if ((int64_t)B * gx * gy >= (int64_t)1 << 31 || (int64_t)B * F >= (int64_t)1 << 31) return api_fail((n + "problem too large").c_str());
    l.B = B; l.K = K; l.H = H; l.W = W; l.F = F; l.gx = (int)gx; l.gy = (int)gy;
    l.face = face; l.bary = bary; l.opacity = faces_opacity; l.scale = face_scale;
    return 0;
}
// rows of C channels at `base` may be read as float4
inline int shade_vec(int C, const float* base) { return (C % 4 == 0 && (reinterpret_cast<uintptr_t>(base) & 15u) == 0u) ? 1 : 0; }

// f(std::integral_constant<int, KMAX>) with the backward kernels' KMAX for lists of K slots: 4 / 8 / 16 / 32
template <class Fn>
void with_kmax(int K, Fn&& f) {
    if (K <= 4) f(std::integral_constant<int, 4>());
    else if (K <= 8) f(std::integral_constant<int, 8>());
    else if (K <= 16) f(std::integral_constant<int, 16>());
    else f(std::integral_constant<int, 32>());
}
// non-zero, with the error set, when the launch before it failed
inline int launched(const char* name) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return api_fail((std::string(name) + ": " + hipGetErrorString(e)).c_str());
    return 0;
}

// What a backward call does before it launches.  The gradient outputs of the lists and the unit's `own` as (pointer, floats),
// null = not wanted, are zeroed on the stream (dL_dbary only without grad_image: else the kernel stores every slot).
// -> SHADE_LAUNCH, SHADE_DONE (no gradient wanted, or the zeros are the gradients) or SHADE_FAILED with the error set.
enum { SHADE_LAUNCH = -1, SHADE_DONE = 0, SHADE_FAILED = 1 };
struct ShadeGrad { float* p; int64_t n; };
template <class P>
int shade_backward_prologue(const char* name, const P& l, const float* grad_image, const float* grad_T, float* dL_dfaces_opacity,
                                   float* dL_dface_scale, float* dL_dbary, std::initializer_list<ShadeGrad> own, hipStream_t st) {
    if (dL_dface_scale && !l.scale) return api_fail((std::string(name) + ": dL_dface_scale without face_scale").c_str());
    bool wanted = dL_dfaces_opacity || dL_dface_scale || dL_dbary;
    for (const ShadeGrad& g : own) wanted = wanted || g.p;
    if (!wanted) return SHADE_DONE;
    hipError_t e = hipSuccess;
    const auto zero = [&](float* q, int64_t n) { if (e == hipSuccess && q && n > 0) e = hipMemsetAsync(q, 0, (size_t)n * sizeof(float), st); };
    zero(dL_dfaces_opacity, l.F);
    for (const ShadeGrad& g : own) zero(g.p, g.n);
    zero(dL_dface_scale, (int64_t)l.B * l.F);
    if (!grad_image) zero(dL_dbary, (int64_t)l.B * l.K * 2 * l.H * l.W);
    if (e != hipSuccess) return api_fail((std::string(name) + ": hipMemsetAsync: " + hipGetErrorString(e)).c_str());
    if (!grad_image && !grad_T) return SHADE_DONE;  // nothing arrives: the zeros are the gradients
    if (!grad_image && !dL_dfaces_opacity) return SHADE_DONE;  // only T's upstream, which reaches the opacities alone
    return SHADE_LAUNCH;
}

}  // namespace dmr
