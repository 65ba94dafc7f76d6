// dmr_visibility.hip -- shading over per-pixel fragment lists (include/dmesh_renderer_amd_visibility.h): per-face visibility
// and coverage, forward and backward.  The models are fragments.face_visibility and fragments.face_coverage (fragments.py);
// what is computed, per pixel over its K slots front to back, f_k the slot's face:
//     o_k = opacity[f_k], T_0 = 1, T_{k+1} = T_k (1 - o_k), w_k = T_k o_k, p = pixel_weight[b, y, x] or 1
//     vis[b, f] = sum of p w_k, max_weight[b, f] = max(0, max of w_k), pixels[b, f] = the number of (pixel, slot) pairs with f_k == f
// A translation unit of its own, as dmr_shade.hip and dmr_texture.hip are: no dmr_scene, no scratch buffer, and it reads the
// face ids and the opacities alone (no barycentrics, no faces, no vertices).  Both kernels use the fragment kernels'
// pixel-to-lane mapping (FragSlots, dmr_device.hpp): one 256-thread workgroup per 16 x 16 tile, 8 x 8 pixels per wave, one
// lane per pixel, so neighbouring lanes mostly hold the same face in the same slot: they merge (shade_merge), the survivors
// add into a per-tile LDS table keyed by face (stab_find), and the table leaves once per tile.
// A slot whose face id lies outside [0, F) is empty wherever it sits; the lists' count is not read.
//
// None of the arithmetic here decides an index or a branch another kernel depends on: it may contract to FMA.
#include "dmr_deferred_common.hpp"  // (for its zeroing kernel)
#include "../../include/dmesh_renderer_amd_visibility.h"

namespace dmr {
namespace {

#pragma clang fp contract(fast)

struct VisParams {
    int B, K, H, W, F, gx, gy;
    const int32_t* __restrict__ face;     // [B,K,H,W]
    const float* __restrict__ opacity;    // [F]
    const float* __restrict__ weight;     // [B,H,W] or null
};

// The per-tile table: face -> the sum of p w_k in an f64 cell (as the other units' tables: an f64 LDS add on distinct cells
// costs a tenth of an f32 one on this part, profiles/r02/lds_atomics.txt) and, with COVERAGE, the largest w_k as the bit
// pattern of a float >= +0 (unsigned order is then the floats' order) and the count.  11 KB with COVERAGE, 6.6 KB without.
template <bool COVERAGE>
struct VisLds {
    double val[STAB];
    uint32_t key[STAB];
    uint32_t mx[COVERAGE ? STAB : 1];
    uint32_t cnt[COVERAGE ? STAB : 1];
};

// ---------------------------------------------------------------------------
// Forward.  One workgroup per tile; a lane walks its pixel's list once, front to back, T in a register.  Per slot the key is
// the face (-1: empty) and the values p w_k and, with COVERAGE, 1 (a float count is exact: at most 16 lanes merge) and w_k for
// the maximum, which merges on a copy of the key (shade_merge_max).  Without COVERAGE a slot whose value is 0 has nothing to
// add and retires before the merge; with it every slot of a face counts.  Rows the table refuses leave with direct atomics.
// Every lane of the workgroup runs every slot (merges, barriers): those outside the image with key -1.
// ---------------------------------------------------------------------------
template <bool COVERAGE>
__global__ void __launch_bounds__(256)
k_face_visibility(VisParams p, float* __restrict__ vis, float* __restrict__ maxw, int32_t* __restrict__ pixels) {
    const int tid = threadIdx.x, lane = tid & 63;
    const auto [tx, ty, b] = tile_coords((int)blockIdx.x, p.gx, p.gy);
    const FragSlots S(tx, ty, b, p.K, p.W, p.H);
    __shared__ VisLds<COVERAGE> L;
    for (int i = tid; i < STAB; i += 256) {
        L.key[i] = STAB_EMPTY;
        L.val[i] = 0.0;
        if constexpr (COVERAGE) { L.mx[i] = 0u; L.cnt[i] = 0u; }
    }
    __syncthreads();
    const float pw = (p.weight && S.inside) ? p.weight[(int64_t)b * S.HW + (int64_t)p.W * S.py + S.px] : 1.f;
    const int64_t row = (int64_t)b * p.F;
    float T = 1.f;
    int nface = S.inside ? p.face[S.face_at(0)] : -1;
    for (int k = 0; k < p.K; k++) {
        const int face = nface;
        if (k + 1 < p.K) nface = S.inside ? p.face[S.face_at(k + 1)] : -1;
        int key = -1;
        float g[COVERAGE ? 2 : 1];
        g[0] = 0.f;
        if constexpr (COVERAGE) g[1] = 0.f;
        float m = 0.f;
        if ((uint32_t)face < (uint32_t)p.F) {
            const float o = p.opacity[face];
            const float w = T * o;
            T = T * (1.f - o);
            g[0] = pw * w;
            if constexpr (COVERAGE) {
                key = face;
                g[1] = 1.f;
                m = w > 0.f ? w : 0.f;  // (+0 for a weight that is negative, -0 or no number: the bit pattern orders as unsigned)
            } else if (g[0] != 0.f) key = face;
        }
        if (__ballot(key >= 0) == 0ull) continue;  // (wave-uniform)
        if constexpr (COVERAGE) shade_merge_max(lane, key, m);
        shade_merge(lane, key, g);
        if (key < 0) continue;
        const int slot = stab_find(L.key, (uint32_t)face);
        if (slot >= 0) {
            atomicAdd(&L.val[slot], (double)g[0]);
            if constexpr (COVERAGE) { atomicMax(&L.mx[slot], __float_as_uint(m)); atomicAdd(&L.cnt[slot], (uint32_t)g[1]); }
        } else {
            unsafeAtomicAdd(&vis[row + face], g[0]);
            if constexpr (COVERAGE) {
                atomicMax(reinterpret_cast<uint32_t*>(&maxw[row + face]), __float_as_uint(m));
                atomicAdd(&pixels[row + face], (int32_t)g[1]);
            }
        }
    }
    __syncthreads();
    for (int slot = tid; slot < STAB; slot += 256) {
        const uint32_t rid = L.key[slot];
        if (rid == STAB_EMPTY) continue;
        unsafeAtomicAdd(&vis[row + rid], (float)L.val[slot]);
        if constexpr (COVERAGE) {
            atomicMax(reinterpret_cast<uint32_t*>(&maxw[row + rid]), L.mx[slot]);
            atomicAdd(&pixels[row + rid], (int32_t)L.cnt[slot]);
        }
    }
}

// ---------------------------------------------------------------------------
// Backward.  T_k of every slot of the tile's pixels (what the recurrence needs from the front-to-back walk) and the table:
// 4 KB + 6.6 KB (KMAX 4) ... 32 KB + 6.6 KB (KMAX 32).
// ---------------------------------------------------------------------------
template <int KMAX>
struct VisBackwardLds {
    float tv[KMAX][TILE_PIX];
    double val[STAB];
    uint32_t key[STAB];
};

// One workgroup per tile, a lane owns its pixel.  With G_k = grad_vis[b, f_k] (0 in empty slots):
//   walk 0 (front to back): T_k of every slot -> LDS.
//   back to front: dL/do_k = p T_k (G_k - R_k), R_{K-1} = 0, R_{k-1} = o_k G_k + (1 - o_k) R_k (composite's opacity recurrence
//     with one channel, a_k = 1, s_k = G_k and no upstream of T; exact for opacities 0 and 1: nothing divides by 1 - o), merged
//     by face, into the table, which leaves once; dL/dp += w_k G_k, one plain store per pixel.
// dop / dpw null: not wanted, and its part is skipped.  Every lane of the workgroup runs every slot (merges, barriers).
template <int KMAX>
__global__ void __launch_bounds__(256)
k_face_visibility_backward(VisParams p, const float* __restrict__ gvis, float* __restrict__ dop, float* __restrict__ dpw) {
    const int tid = threadIdx.x, lane = tid & 63;
    const auto [tx, ty, b] = tile_coords((int)blockIdx.x, p.gx, p.gy);
    const FragSlots S(tx, ty, b, p.K, p.W, p.H);
    const int64_t pix = (int64_t)b * S.HW + (int64_t)p.W * S.py + S.px;
    __shared__ VisBackwardLds<KMAX> L;
    for (int i = tid; i < STAB; i += 256) { L.key[i] = STAB_EMPTY; L.val[i] = 0.0; }
    {
        float T = 1.f;
        for (int k = 0; k < p.K; k++) {
            const int face = S.inside ? p.face[S.face_at(k)] : -1;
            L.tv[k][tid] = T;
            if ((uint32_t)face < (uint32_t)p.F) T = T * (1.f - p.opacity[face]);
        }
    }
    __syncthreads();
    const float pw = (p.weight && S.inside) ? p.weight[pix] : 1.f;
    const int64_t row = (int64_t)b * p.F;
    float R = 0.f, dp = 0.f;
    for (int k = p.K - 1; k >= 0; k--) {
        const int face = S.inside ? p.face[S.face_at(k)] : -1;
        int key = -1;
        float fg[1] = {0.f};  // dL/do_k
        if ((uint32_t)face < (uint32_t)p.F) {
            const float o = p.opacity[face], T = L.tv[k][tid], G = gvis[row + face];
            fg[0] = pw * T * (G - R);
            dp += T * o * G;
            R = o * G + (1.f - o) * R;
            if (dop && fg[0] != 0.f) key = face;
        }
        if (__ballot(key >= 0) == 0ull) continue;  // (wave-uniform)
        shade_merge(lane, key, fg);
        if (key < 0) continue;
        const int slot = stab_find(L.key, (uint32_t)face);
        if (slot >= 0) atomicAdd(&L.val[slot], (double)fg[0]);
        else unsafeAtomicAdd(&dop[face], fg[0]);
    }
    if (dpw && S.inside) dpw[pix] = dp;
    if (!dop) return;  // uniform
    __syncthreads();
    for (int slot = tid; slot < STAB; slot += 256) {
        const uint32_t rid = L.key[slot];
        if (rid != STAB_EMPTY) unsafeAtomicAdd(&dop[rid], (float)L.val[slot]);
    }
}

#pragma clang fp contract(off)

// the arguments both calls share -> VisParams; non-zero with the error set.  (shade_check_lists asks for barycentrics and a
// corner table, which this unit does not read: the list check here is its own.)
int vis_params(const char* name, int B, int K, int H, int W, int F, const int32_t* face, const float* faces_opacity,
               const float* pixel_weight, VisParams& p) {
    const std::string n = std::string(name) + ": ";
    if (shade_check_sizes(n, B, K, H, W, 0, F, 1, 1)) return 1;
    if (!face) return api_fail((n + "null fragment lists").c_str());
    if (F > 0 && !faces_opacity) return api_fail((n + "null faces_opacity").c_str());
    const int64_t gx = (W + TILE - 1) / TILE, gy = (H + TILE - 1) / TILE;
    if ((int64_t)B * gx * gy >= (int64_t)1 << 31 || (int64_t)B * F >= (int64_t)1 << 31 || (int64_t)K * H * W >= (int64_t)1 << 31)
        return api_fail((n + "problem too large").c_str());
    p.B = B; p.K = K; p.H = H; p.W = W; p.F = F; p.gx = (int)gx; p.gy = (int)gy;
    p.face = face; p.opacity = faces_opacity; p.weight = pixel_weight;
    return 0;
}

}  // namespace
}  // namespace dmr

extern "C" {

int dmr_face_visibility(int B, int K, int H, int W, int F, const int32_t* face, const float* faces_opacity,
                        const float* pixel_weight, float* vis, float* max_weight, int32_t* pixels, void* stream) {
    using namespace dmr;
    const char* name = "dmr_face_visibility";
    VisParams p;
    if (vis_params(name, B, K, H, W, F, face, faces_opacity, pixel_weight, p)) return 1;
    if ((max_weight == nullptr) != (pixels == nullptr)) return api_fail("dmr_face_visibility: max_weight and pixels go together: both or neither");
    if (F == 0) return 0;  // [B,0] outputs: nothing to write
    if (!vis) return api_fail("dmr_face_visibility: null output");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int64_t n = (int64_t)B * F;
    zero_on(st, vis, n, max_weight, n, pixels, n);  // (k_deferred_zero, dmr_deferred_common.hpp: a kernel, not hipMemsetAsync -- DESIGN.md 5e)
    if (launched(name)) return 1;
    const dim3 grid((unsigned)(B * p.gx * p.gy)), block(256);
    if (max_weight) k_face_visibility<true><<<grid, block, 0, st>>>(p, vis, max_weight, pixels);
    else k_face_visibility<false><<<grid, block, 0, st>>>(p, vis, nullptr, nullptr);
    return launched(name);
}

int dmr_face_visibility_backward(int B, int K, int H, int W, int F, const int32_t* face, const float* faces_opacity,
                                 const float* pixel_weight, const float* grad_vis, float* dL_dfaces_opacity,
                                 float* dL_dpixel_weight, void* stream) {
    using namespace dmr;
    const char* name = "dmr_face_visibility_backward";
    VisParams p;
    if (vis_params(name, B, K, H, W, F, face, faces_opacity, pixel_weight, p)) return 1;
    if (F > 0 && !grad_vis) return api_fail("dmr_face_visibility_backward: null grad_vis");
    if (dL_dpixel_weight && !pixel_weight) return api_fail("dmr_face_visibility_backward: dL_dpixel_weight without pixel_weight");
    if (!dL_dfaces_opacity && !dL_dpixel_weight) return 0;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    zero_on(st, dL_dfaces_opacity, F, nullptr, 0, nullptr, 0);  // (one buffer for all views: the tiles add into it)
    if (launched(name)) return 1;
    if (F == 0 && !dL_dpixel_weight) return 0;
    // (F == 0 with dL_dpixel_weight: every slot is empty, and the kernel stores the zeros)
    float* dop = F > 0 ? dL_dfaces_opacity : nullptr;
    with_kmax(K, [&](auto kmax) {
        k_face_visibility_backward<decltype(kmax)::value><<<dim3((unsigned)(B * p.gx * p.gy)), dim3(256), 0, st>>>(p, grad_vis, dop, dL_dpixel_weight);
    });
    return launched(name);
}

}  // extern "C"
