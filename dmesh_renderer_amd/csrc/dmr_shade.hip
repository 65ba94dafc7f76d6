// dmr_shade.hip -- shading over per-pixel fragment lists (include/dmesh_renderer_amd_shade.h): the fused compositing of
// per-vertex attributes, forward and backward.  The model is fragments.composite (fragments.py); what is computed:
//     o_k = opacity[face_k], T_0 = 1, T_{k+1} = T_k (1 - o_k), w_k = T_k o_k, a_k = (1 - u - v) A[v0] + u A[v1] + v A[v2],
//     image = sum_k w_k s_k a_k, T = T_K                                 (s_k = face_scale[b, face_k] or 1)
// A translation unit of its own: it takes no dmr_scene and no scratch buffer, and the renderers' kernels compile as they did
// without it.  Both kernels use the fragment kernels' pixel-to-lane mapping (FragSlots, dmr_device.hpp): one 256-thread
// workgroup per 16 x 16 tile, 8 x 8 pixels per wave, one lane per pixel, so neighbouring lanes mostly gather the same rows.
// A slot whose face id lies outside [0, F) is empty wherever it sits; the lists' count is not read.
//
// None of the arithmetic here decides an index or a branch another kernel depends on: it may contract to FMA.
#include "dmr_shade_common.hpp"
#include "../../include/dmesh_renderer_amd_shade.h"

namespace dmr {
namespace {

#pragma clang fp contract(fast)

constexpr int SHADE_MAX_C = 256;

struct ShadeParams {
    int B, K, H, W, P, F, C, gx, gy;
    int vec;  // rows of vert_attrs may be read as float4 (C % 4 == 0, 16-byte aligned base)
    const int32_t* __restrict__ face;     // [B,K,H,W]
    const float* __restrict__ bary;       // [B,K,2,H,W]
    const int32_t* __restrict__ faces;    // [F,3]
    const float* __restrict__ opacity;    // [F]
    const float* __restrict__ attrs;      // [P,C]
    const float* __restrict__ scale;      // [B,F] or null
};

// channels c0 .. c0 + CH - 1 of row v of vert_attrs (0 past C)
template <int CH>
__device__ __forceinline__ void load_row(const ShadeParams& p, int v, int c0, float (&r)[CH]) {
    static_assert(CH % 4 == 0, "whole float4");
    const float* __restrict__ row = p.attrs + (int64_t)v * p.C + c0;
    if (p.vec) {
#pragma unroll
        for (int i = 0; i < CH / 4; i++) {
            float4 t = {0.f, 0.f, 0.f, 0.f};
            if (c0 + 4 * i < p.C) t = *reinterpret_cast<const float4*>(row + 4 * i);
            r[4 * i] = t.x; r[4 * i + 1] = t.y; r[4 * i + 2] = t.z; r[4 * i + 3] = t.w;
        }
    } else {
#pragma unroll
        for (int c = 0; c < CH; c++) r[c] = c0 + c < p.C ? row[c] : 0.f;
    }
}

// The three vertices of a face; false when one of them is no row of vert_attrs (such a slot gathers and scatters nothing).
__device__ __forceinline__ bool face_verts(const ShadeParams& p, int face, int (&v)[3]) {
    v[0] = p.faces[3 * face]; v[1] = p.faces[3 * face + 1]; v[2] = p.faces[3 * face + 2];
    return (uint32_t)v[0] < (uint32_t)p.P && (uint32_t)v[1] < (uint32_t)p.P && (uint32_t)v[2] < (uint32_t)p.P;
}

// ---------------------------------------------------------------------------
// Forward.  A lane walks its pixel's list once per chunk of CH channels, the chunk's accumulators in registers: any C works
// without spills (C <= 4: one walk with CH = 4; else CH = 16).  A slot of weight 0 -- empty, opacity 0, or behind a face of
// opacity 1 -- gathers nothing.  No LDS, no barrier: lanes outside the image leave at once.
// ---------------------------------------------------------------------------
template <int CH>
__global__ void __launch_bounds__(256)
k_composite_fragments(ShadeParams p, float* __restrict__ image, float* __restrict__ Tout) {
    const auto [tx, ty, b] = tile_coords((int)blockIdx.x, p.gx, p.gy);
    const FragSlots S(tx, ty, b, p.K, p.W, p.H);
    if (!S.inside) return;
    const int64_t pix = (int64_t)p.W * S.py + S.px;
    for (int c0 = 0; c0 < p.C; c0 += CH) {
        float acc[CH];
#pragma unroll
        for (int c = 0; c < CH; c++) acc[c] = 0.f;
        float T = 1.f;
        int nface = p.face[S.face_at(0)];
        for (int k = 0; k < p.K; k++) {
            const int face = nface;
            if (k + 1 < p.K) nface = p.face[S.face_at(k + 1)];
            if ((uint32_t)face >= (uint32_t)p.F) continue;
            const float o = p.opacity[face];
            const float w = T * o;
            T = T * (1.f - o);
            if (w == 0.f) continue;
            int v[3];
            if (!face_verts(p, face, v)) continue;
            const float q = p.scale ? w * p.scale[(int64_t)b * p.F + face] : w;
            const float bu = p.bary[S.grad_at(k, 0)], bv = p.bary[S.grad_at(k, 1)];
            const float b0 = 1.f - bu - bv;
            float r0[CH], r1[CH], r2[CH];
            load_row<CH>(p, v[0], c0, r0); load_row<CH>(p, v[1], c0, r1); load_row<CH>(p, v[2], c0, r2);
#pragma unroll
            for (int c = 0; c < CH; c++) acc[c] += q * (b0 * r0[c] + bu * r1[c] + bv * r2[c]);
        }
#pragma unroll
        for (int c = 0; c < CH; c++)
            if (c0 + c < p.C) image[((int64_t)b * p.C + c0 + c) * S.HW + pix] = acc[c];
        if (c0 == 0) Tout[(int64_t)b * S.HW + pix] = T;
    }
}

// ---------------------------------------------------------------------------
// Backward.
//
// Lanes that hold the same key (a face) merge before they go to the table (shade_merge, stab_find: dmr_shade_common.hpp).
// ---------------------------------------------------------------------------

// T_k and e_k = a_k . g of every slot of the tile's pixels (what the opacity recurrence needs from the front-to-back walk),
// and the table: key -> CH sums, in f64 cells as k_tri_backward_hits' table: on this part an f32 LDS add costs about 3 cycles
// per lane per CU, an f64 one a tenth of that on distinct cells (profiles/r02/lds_atomics.txt).  KMAX = 4 / 8 / 16 / 32 slots,
// CH = 4 / 8 channels per walk: 8 KB + 20 KB (KMAX 4, CH 4) ... 64 KB + 38 KB (KMAX 32, CH 8).
template <int KMAX, int CH>
struct ShadeLds {
    float tv[KMAX][TILE_PIX];
    float ev[KMAX][TILE_PIX];
    double val[STAB][CH];
    uint32_t key[STAB];
};

// One workgroup per tile, a lane owns its pixel.  With g the pixel's upstream of the image, gT that of T:
//   walk 0 (front to back, no gathers): T_k of every slot -> LDS.
//   per chunk of CH channels, front to back: e_k += a_k . g (LDS), dL/dbary (u: w s (A[v1] - A[v0]) . g, v alike; the lane is
//     the slot's one writer: the first chunk stores, later ones add), and the rows w s beta_j g of the three vertices:
//     merged over the wave's lanes of equal face, then into the table keyed by vertex, which leaves once per chunk.
//   last walk, back to front: d_k = s_k e_k, dL/do_k = T_k (d_k - R_k), R_{K-1} = gT, R_{k-1} = o_k d_k + (1 - o_k) R_k (exact
//     for opacities 0 and 1: nothing divides by 1 - o), dL/ds_k = w_k e_k; merged by face, into the table re-keyed by face.
// Slots behind a face of opacity 1 (T_k = 0) gather nothing unless dL/do is wanted.  Every lane of the workgroup runs every
// walk (merges, barriers).
template <int KMAX, int CH>
__global__ void __launch_bounds__(256)
k_composite_fragments_backward(ShadeParams p, const float* __restrict__ gimg, const float* __restrict__ gT, float* __restrict__ dop,
                               float* __restrict__ dattr, float* __restrict__ dsc, float* __restrict__ dbary) {
    const int tid = threadIdx.x, lane = tid & 63;
    const auto [tx, ty, b] = tile_coords((int)blockIdx.x, p.gx, p.gy);
    const FragSlots S(tx, ty, b, p.K, p.W, p.H);
    const int64_t pix = (int64_t)p.W * S.py + S.px;
    __shared__ ShadeLds<KMAX, CH> L;
    for (int i = tid; i < STAB; i += 256) {
        L.key[i] = STAB_EMPTY;
#pragma unroll
        for (int c = 0; c < CH; c++) L.val[i][c] = 0.0;
    }
    {
        float T = 1.f;
        for (int k = 0; k < p.K; k++) {
            const int face = S.inside ? p.face[S.face_at(k)] : -1;
            L.tv[k][tid] = T; L.ev[k][tid] = 0.f;
            if ((uint32_t)face < (uint32_t)p.F) T = T * (1.f - p.opacity[face]);
        }
    }
    __syncthreads();
    const bool need_e = dop || dsc || dbary;
    if (gimg) {
        for (int c0 = 0; c0 < p.C; c0 += CH) {
            float g[CH];
#pragma unroll
            for (int c = 0; c < CH; c++) g[c] = (S.inside && c0 + c < p.C) ? gimg[((int64_t)b * p.C + c0 + c) * S.HW + pix] : 0.f;
            for (int k = 0; k < p.K; k++) {
                const int face = S.inside ? p.face[S.face_at(k)] : -1;
                int key = -1, v[3] = {0, 0, 0};
                float du = 0.f, dv = 0.f;
                float rows[3 * CH];
#pragma unroll
                for (int c = 0; c < 3 * CH; c++) rows[c] = 0.f;
                const float T = L.tv[k][tid];
                // (a slot behind a face of opacity 1, T_k = 0, still has its e_k read by that face's dL/do: what it would uncover)
                if ((uint32_t)face < (uint32_t)p.F && (T != 0.f || dop) && face_verts(p, face, v)) {
                    const float q = T * p.opacity[face] * (p.scale ? p.scale[(int64_t)b * p.F + face] : 1.f);
                    const float bu = p.bary[S.grad_at(k, 0)], bv = p.bary[S.grad_at(k, 1)];
                    const float b0 = 1.f - bu - bv;
                    if (need_e) {
                        float r0[CH], r1[CH], r2[CH];
                        load_row<CH>(p, v[0], c0, r0); load_row<CH>(p, v[1], c0, r1); load_row<CH>(p, v[2], c0, r2);
                        float e0 = 0.f, e1 = 0.f, e2 = 0.f;
#pragma unroll
                        for (int c = 0; c < CH; c++) { e0 += r0[c] * g[c]; e1 += r1[c] * g[c]; e2 += r2[c] * g[c]; }
                        L.ev[k][tid] += b0 * e0 + bu * e1 + bv * e2;
                        du = q * (e1 - e0); dv = q * (e2 - e0);
                    }
                    if (dattr && q != 0.f) {
                        key = face;
#pragma unroll
                        for (int c = 0; c < CH; c++) { rows[c] = q * b0 * g[c]; rows[CH + c] = q * bu * g[c]; rows[2 * CH + c] = q * bv * g[c]; }
                    }
                }
                if (dbary && S.inside) {
                    if (c0 == 0) { dbary[S.grad_at(k, 0)] = du; dbary[S.grad_at(k, 1)] = dv; }
                    else if (du != 0.f || dv != 0.f) { dbary[S.grad_at(k, 0)] += du; dbary[S.grad_at(k, 1)] += dv; }
                }
                if (!dattr || __ballot(key >= 0) == 0ull) continue;  // (wave-uniform)
                shade_merge(lane, key, rows);
                if (key < 0) continue;
                // (lanes of equal face hold equal vertices: v is the merged rows' too)
#pragma unroll
                for (int j = 0; j < 3; j++) {
                    const int slot = stab_find(L.key, (uint32_t)v[j]);
#pragma unroll
                    for (int c = 0; c < CH; c++) {
                        if (c0 + c >= p.C) continue;
                        if (slot >= 0) atomicAdd(&L.val[slot][c], (double)rows[j * CH + c]);
                        else unsafeAtomicAdd(&dattr[(int64_t)v[j] * p.C + c0 + c], rows[j * CH + c]);
                    }
                }
            }
            if (dattr) {  // the chunk's table leaves: CH lanes per slot; the keys stay for the next chunk
                __syncthreads();
                for (int i = tid; i < STAB * CH; i += 256) {
                    const int slot = i / CH, c = i % CH;
                    const uint32_t rid = L.key[slot];
                    const double x = L.val[slot][c];
                    if (rid != STAB_EMPTY && x != 0.0) {
                        L.val[slot][c] = 0.0;
                        if (c0 + c < p.C) unsafeAtomicAdd(&dattr[(int64_t)rid * p.C + c0 + c], (float)x);
                    }
                }
                __syncthreads();
            }
        }
    }
    if (!dop && !dsc) return;  // uniform
    __syncthreads();
    for (int i = tid; i < STAB; i += 256) L.key[i] = STAB_EMPTY;  // (the values are zero: every chunk's flush left them so)
    __syncthreads();
    float R = (gT && S.inside) ? gT[(int64_t)b * S.HW + pix] : 0.f;
    for (int k = p.K - 1; k >= 0; k--) {
        const int face = S.inside ? p.face[S.face_at(k)] : -1;
        int key = -1;
        float fg[2] = {0.f, 0.f};  // dL/do_k, dL/ds_k
        if ((uint32_t)face < (uint32_t)p.F) {
            const float o = p.opacity[face], T = L.tv[k][tid], e = L.ev[k][tid];
            const float d = p.scale ? p.scale[(int64_t)b * p.F + face] * e : e;
            fg[0] = T * (d - R);
            fg[1] = T * o * e;
            R = o * d + (1.f - o) * R;
            if (fg[0] != 0.f || fg[1] != 0.f) key = face;
        }
        if (__ballot(key >= 0) == 0ull) continue;  // (wave-uniform)
        shade_merge(lane, key, fg);
        if (key < 0) continue;
        const int slot = stab_find(L.key, (uint32_t)face);
        if (slot >= 0) { atomicAdd(&L.val[slot][0], (double)fg[0]); atomicAdd(&L.val[slot][1], (double)fg[1]); }
        else {
            if (dop) unsafeAtomicAdd(&dop[face], fg[0]);
            if (dsc) unsafeAtomicAdd(&dsc[(int64_t)b * p.F + face], fg[1]);
        }
    }
    __syncthreads();
    for (int slot = tid; slot < STAB; slot += 256) {
        const uint32_t rid = L.key[slot];
        if (rid == STAB_EMPTY) continue;
        if (dop) unsafeAtomicAdd(&dop[rid], (float)L.val[slot][0]);
        if (dsc) unsafeAtomicAdd(&dsc[(int64_t)b * p.F + rid], (float)L.val[slot][1]);
    }
}

#pragma clang fp contract(off)

// the arguments both calls share -> ShadeParams; non-zero with the error set
int shade_params(const char* name, int B, int K, int H, int W, int P, int F, int C, const int32_t* face, const float* bary,
                 const int32_t* faces, const float* faces_opacity, const float* vert_attrs, const float* face_scale, ShadeParams& p) {
    const std::string n = std::string(name) + ": ";
    if (shade_check_sizes(n, B, K, H, W, P, F, C, SHADE_MAX_C)) return 1;
    const char* missing = (F > 0 && P > 0 && !vert_attrs) ? "vert_attrs" : nullptr;
    if (shade_check_lists(n, "faces", B, K, H, W, F, face, bary, faces, faces_opacity, face_scale, missing, p)) return 1;
    p.P = P; p.C = C;
    p.vec = shade_vec(C, vert_attrs);
    p.faces = faces; p.attrs = vert_attrs;
    return 0;
}

template <int KMAX>
void launch_backward(const ShadeParams& p, hipStream_t st, const float* gi, const float* gt, float* dop, float* dattr,
                     float* dsc, float* dbary) {
    if (p.C <= 4) k_composite_fragments_backward<KMAX, 4><<<dim3((unsigned)(p.B * p.gx * p.gy)), dim3(256), 0, st>>>(p, gi, gt, dop, dattr, dsc, dbary);
    else k_composite_fragments_backward<KMAX, 8><<<dim3((unsigned)(p.B * p.gx * p.gy)), dim3(256), 0, st>>>(p, gi, gt, dop, dattr, dsc, dbary);
}

}  // namespace
}  // namespace dmr

extern "C" {

int dmr_composite_fragments(int B, int K, int H, int W, int P, int F, int C, const int32_t* face, const float* bary,
                            const int32_t* faces, const float* faces_opacity, const float* vert_attrs, const float* face_scale,
                            float* image, float* T, void* stream) {
    using namespace dmr;
    ShadeParams p;
    if (shade_params("dmr_composite_fragments", B, K, H, W, P, F, C, face, bary, faces, faces_opacity, vert_attrs, face_scale, p)) return 1;
    if (!image || !T) return api_fail("dmr_composite_fragments: null output");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)(B * p.gx * p.gy)), block(256);
    if (C <= 4) k_composite_fragments<4><<<grid, block, 0, st>>>(p, image, T);
    else k_composite_fragments<16><<<grid, block, 0, st>>>(p, image, T);
    return launched("dmr_composite_fragments");
}

int dmr_composite_fragments_backward(int B, int K, int H, int W, int P, int F, int C, const int32_t* face, const float* bary,
                                     const int32_t* faces, const float* faces_opacity, const float* vert_attrs,
                                     const float* face_scale, const float* grad_image, const float* grad_T,
                                     float* dL_dfaces_opacity, float* dL_dvert_attrs, float* dL_dface_scale, float* dL_dbary,
                                     void* stream) {
    using namespace dmr;
    const char* name = "dmr_composite_fragments_backward";
    ShadeParams p;
    if (shade_params(name, B, K, H, W, P, F, C, face, bary, faces, faces_opacity, vert_attrs, face_scale, p)) return 1;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int r = shade_backward_prologue(name, p, grad_image, grad_T, dL_dfaces_opacity, dL_dface_scale, dL_dbary,
                                          {{dL_dvert_attrs, (int64_t)P * C}}, st);
    if (r != SHADE_LAUNCH) return r;
    with_kmax(K, [&](auto kmax) {
        launch_backward<decltype(kmax)::value>(p, st, grad_image, grad_T, dL_dfaces_opacity, dL_dvert_attrs, dL_dface_scale, dL_dbary);
    });
    return launched(name);
}

}  // extern "C"
