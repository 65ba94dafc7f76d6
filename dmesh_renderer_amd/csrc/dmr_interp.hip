// dmr_interp.hip -- shading over per-pixel fragment lists (include/dmesh_renderer_amd_deferred.h): the two ends of a deferred
// shader, each forward and backward.  The models are fragments.interpolate and fragments.composite_values (fragments.py):
//     interpolate:  out[b,k,c] = (1 - u - v) A[v0][c] + u A[v1][c] + v A[v2][c], (v0, v1, v2) = faces[face_k]; 0 in empty slots
//     composite:    o_k = opacity[face_k], T_0 = 1, T_{k+1} = T_k (1 - o_k), w_k = T_k o_k, s_k = face_scale[b, face_k] or 1,
//                   image[b,c] = sum_k w_k s_k values[b,k,c], T = T_K
// between which the caller runs its own code on every fragment.  A translation unit of its own, as the other shading units
// are: no dmr_scene, no scratch buffer.  out, values and their gradients are [B,K,C,H,W] planes: B K C H W passes 2^31 at real
// sizes, so every offset into them is an int64_t.
//
// What this unit shares with its packed twin (dmr_packed.hip) -- the lane mappings, the backward kernels' LDS tables, the
// vertex lookup, the zeroing kernel, the host checks -- is stated once, in dmr_deferred_common.hpp; the walks and the row load
// (interp_row) are this unit's own text.
// Two pixel-to-lane mappings, RowPix and TilePix.  The two forwards merge nothing and stream B K C H W floats: they use
// RowPix, a wave on 64 pixels of one image row, so that a plane is touched in 256 contiguous bytes per wave-instruction.  The two
// backward kernels merge lanes of equal face (shade_merge) and sum in a per-workgroup LDS table (stab_find); each runs on the
// mapping it measured faster on (profiles/deferred/lane_shapes.txt): the interpolation's, which merges 3 CH values
// per slot, on the fragment kernels' 8 x 8 pixels per wave (TilePix = FragSlots, dmr_device.hpp), the blend's, which stores
// dL/dvalues for every slot and merges two values, on RowPix.
// A slot whose face id lies outside [0, F) is empty wherever it sits; the lists' count is not read.
//
// None of the arithmetic here decides an index or a branch another kernel depends on: it may contract to FMA.
#include "dmr_deferred_common.hpp"
#include "../../include/dmesh_renderer_amd_deferred.h"

namespace dmr {
namespace {

#pragma clang fp contract(fast)

constexpr int DEFER_MAX_C = 256;

struct InterpParams {
    int B, K, H, W, P, F, C, gx, gy, sx, sy;
    int vec;  // rows of vert_attrs may be read as float4 (C % 4 == 0, 16-byte aligned base)
    const int32_t* __restrict__ face;     // [B,K,H,W]
    const float* __restrict__ bary;       // [B,K,2,H,W]
    const int32_t* __restrict__ faces;    // [F,3]
    const float* __restrict__ attrs;      // [P,C]
};

struct ValuesParams {
    int B, K, H, W, F, C, gx, gy, sx, sy;
    const int32_t* __restrict__ face;     // [B,K,H,W]
    const float* __restrict__ opacity;    // [F]
    const float* __restrict__ values;     // [B,K,C,H,W]
    const float* __restrict__ scale;      // [B,F] or null
};

// channels c0 .. c0 + CH - 1 of row v of vert_attrs (0 past C)
template <int CH>
__device__ __forceinline__ void interp_row(const InterpParams& p, int v, int c0, float (&r)[CH]) {
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

// ---------------------------------------------------------------------------
// interpolate, forward.  One lane per pixel (RowPix); per slot the three vertex ids and the weights once, then the channels in
// chunks of CH, every one a plain store: an empty slot (and a face with a vertex that is no row) stores exact zeros.  No LDS, no
// barrier: lanes outside the image leave at once.
// ---------------------------------------------------------------------------
template <int CH>
__global__ void __launch_bounds__(256)
k_interpolate_fragments(InterpParams p, float* __restrict__ out) {
    const RowPix S((int)blockIdx.x, p.sx, p.sy, p.W, p.H);
    if (!S.inside) return;
    int nface = p.face[(int64_t)S.b * p.K * S.HW + S.pix];
    for (int k = 0; k < p.K; k++) {
        const int64_t slot = (int64_t)S.b * p.K + k;
        const int face = nface;
        if (k + 1 < p.K) nface = p.face[(slot + 1) * S.HW + S.pix];
        int v[3] = {0, 0, 0};
        const bool used = (uint32_t)face < (uint32_t)p.F && interp_verts(p, face, v);
        float bu = 0.f, bv = 0.f;
        if (used) { bu = p.bary[(2 * slot) * S.HW + S.pix]; bv = p.bary[(2 * slot + 1) * S.HW + S.pix]; }
        const float b0 = 1.f - bu - bv;
        float* __restrict__ o = out + slot * p.C * S.HW + S.pix;
        for (int c0 = 0; c0 < p.C; c0 += CH) {
            float a[CH];
#pragma unroll
            for (int c = 0; c < CH; c++) a[c] = 0.f;
            if (used) {
                float r0[CH], r1[CH], r2[CH];
                interp_row<CH>(p, v[0], c0, r0); interp_row<CH>(p, v[1], c0, r1); interp_row<CH>(p, v[2], c0, r2);
#pragma unroll
                for (int c = 0; c < CH; c++) a[c] = b0 * r0[c] + bu * r1[c] + bv * r2[c];
            }
#pragma unroll
            for (int c = 0; c < CH; c++)
                if (c0 + c < p.C) o[(int64_t)(c0 + c) * S.HW] = a[c];
        }
    }
}

// ---------------------------------------------------------------------------
// interpolate, backward.  The per-tile table is InterpLds<CH> (dmr_deferred_common.hpp).
// ---------------------------------------------------------------------------
// One workgroup per tile, a lane owns its pixel (InterpBackwardPix).  Per chunk of CH channels, front to back, with g_k the slot's
// upstream: dL/dbary = ((A[v1] - A[v0]) . g_k, (A[v2] - A[v0]) . g_k) (the lane is the slot's one writer: the first chunk
// stores -- an exact 0 in empty slots, so nothing is zeroed beforehand -- later ones add), and the rows beta_j g_k of the three
// vertices: merged over the wave's lanes of equal face, then into the table keyed by vertex, which leaves once per chunk (its
// keys stay).  This is composite's step 2 without the opacity terms.  dattr / dbary null: not wanted, and its part
// is skipped (no rows read without dbary; no merge, no table, no barrier without dattr).  With dattr every lane of the
// workgroup runs every slot (merges, barriers): those outside the image with key -1.
template <int CH>
__global__ void __launch_bounds__(256)
k_interpolate_fragments_backward(InterpParams p, const float* __restrict__ gout, float* __restrict__ dattr, float* __restrict__ dbary) {
    const int tid = threadIdx.x, lane = tid & 63;
    const InterpBackwardPix S((int)blockIdx.x, InterpBackwardPix::nx(p), InterpBackwardPix::ny(p), p.W, p.H);
    const int b = S.b;
    const int64_t pix = S.pix;
    __shared__ InterpLds<CH> L;
    if (dattr) {
        for (int i = tid; i < STAB; i += 256) {
            L.key[i] = STAB_EMPTY;
#pragma unroll
            for (int c = 0; c < CH; c++) L.val[i][c] = 0.0;
        }
        __syncthreads();
    }
    for (int c0 = 0; c0 < p.C; c0 += CH) {
        for (int k = 0; k < p.K; k++) {
            const int64_t slot_at = ((int64_t)b * p.K + k) * S.HW + pix;           // of face [B,K,H,W]
            const int64_t u_at = (2 * ((int64_t)b * p.K + k)) * S.HW + pix, v_at = u_at + S.HW;  // of bary / dL_dbary [B,K,2,H,W]
            const int face = S.inside ? p.face[slot_at] : -1;
            int key = -1, v[3] = {0, 0, 0};
            float du = 0.f, dv = 0.f;
            float rows[3 * CH];
#pragma unroll
            for (int c = 0; c < 3 * CH; c++) rows[c] = 0.f;
            if ((uint32_t)face < (uint32_t)p.F && interp_verts(p, face, v)) {
                const float* __restrict__ gk = gout + (((int64_t)b * p.K + k) * p.C + c0) * S.HW + pix;
                float g[CH];
#pragma unroll
                for (int c = 0; c < CH; c++) g[c] = c0 + c < p.C ? gk[(int64_t)c * S.HW] : 0.f;
                if (dbary) {
                    float r0[CH], r1[CH], r2[CH];
                    interp_row<CH>(p, v[0], c0, r0); interp_row<CH>(p, v[1], c0, r1); interp_row<CH>(p, v[2], c0, r2);
                    float e0 = 0.f, e1 = 0.f, e2 = 0.f;
#pragma unroll
                    for (int c = 0; c < CH; c++) { e0 += r0[c] * g[c]; e1 += r1[c] * g[c]; e2 += r2[c] * g[c]; }
                    du = e1 - e0; dv = e2 - e0;
                }
                if (dattr) {
                    const float bu = p.bary[u_at], bv = p.bary[v_at];
                    const float b0 = 1.f - bu - bv;
                    key = face;
#pragma unroll
                    for (int c = 0; c < CH; c++) { rows[c] = b0 * g[c]; rows[CH + c] = bu * g[c]; rows[2 * CH + c] = bv * g[c]; }
                }
            }
            if (dbary && S.inside) {
                if (c0 == 0) { dbary[u_at] = du; dbary[v_at] = dv; }
                else if (du != 0.f || dv != 0.f) { dbary[u_at] += du; dbary[v_at] += dv; }
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

// ---------------------------------------------------------------------------
// composite_values, forward.  A lane (RowPix) walks its pixel's list once per chunk of CH channels, T and the chunk's
// accumulators in registers (C <= 4: one walk with CH = 4; else CH = 16); per slot one coalesced read of values[b,k,c] per
// channel.  An empty slot and a slot of weight 0 -- opacity 0, or behind a face of opacity 1 -- load nothing.  No LDS, no
// barrier: lanes outside the image leave at once.
// ---------------------------------------------------------------------------
template <int CH>
__global__ void __launch_bounds__(256)
k_composite_values(ValuesParams p, float* __restrict__ image, float* __restrict__ Tout) {
    const RowPix S((int)blockIdx.x, p.sx, p.sy, p.W, p.H);
    if (!S.inside) return;
    const int64_t list = (int64_t)S.b * p.K;
    for (int c0 = 0; c0 < p.C; c0 += CH) {
        float acc[CH];
#pragma unroll
        for (int c = 0; c < CH; c++) acc[c] = 0.f;
        float T = 1.f;
        int nface = p.face[list * S.HW + S.pix];
        for (int k = 0; k < p.K; k++) {
            const int face = nface;
            if (k + 1 < p.K) nface = p.face[(list + k + 1) * S.HW + S.pix];
            if ((uint32_t)face >= (uint32_t)p.F) continue;
            const float o = p.opacity[face];
            const float w = T * o;
            T = T * (1.f - o);
            if (w == 0.f) continue;
            const float q = p.scale ? w * p.scale[(int64_t)S.b * p.F + face] : w;
            const float* __restrict__ vk = p.values + ((list + k) * p.C + c0) * S.HW + S.pix;
#pragma unroll
            for (int c = 0; c < CH; c++)
                if (c0 + c < p.C) acc[c] += q * vk[(int64_t)c * S.HW];
        }
#pragma unroll
        for (int c = 0; c < CH; c++)
            if (c0 + c < p.C) image[((int64_t)S.b * p.C + c0 + c) * S.HW + S.pix] = acc[c];
        if (c0 == 0) Tout[(int64_t)S.b * S.HW + S.pix] = T;
    }
}

// ---------------------------------------------------------------------------
// composite_values, backward.  T_k, e_k and the per-workgroup table are ValuesLds<KMAX> (dmr_deferred_common.hpp).
// ---------------------------------------------------------------------------
// One workgroup per 64 x 4 pixels, a lane owns its pixel (ValuesBackwardPix).  With g the pixel's upstream of the image, gT that of T:
//   walk 0 (front to back, no values): T_k of every slot -> LDS.
//   per chunk of CH channels, front to back: dL/dvalues[b,k,c] = w_k s_k g[c], a plain store to every slot of every pixel of
//     the image (0 in empty slots: nothing is zeroed beforehand), and e_k += values_k . g (LDS) when dL/do or dL/ds is wanted.
//     An empty slot's value is not read; a slot of weight 0 is read only for dL/do (what the face in front of it would uncover).
//   last walk, back to front: d_k = s_k e_k, dL/do_k = T_k (d_k - R_k), R_{K-1} = gT, R_{k-1} = o_k d_k + (1 - o_k) R_k (exact
//     for opacities 0 and 1: nothing divides by 1 - o), dL/ds_k = w_k e_k; merged by face, into the table, which leaves once.
// gimg null: no value is read (the host has zeroed dL/dvalues, and passes dval null).  dop / dval / dsc null: not wanted, and
// its part is skipped.  Every lane of the workgroup runs the last walk (merges, barriers).
template <int KMAX, int CH>
__global__ void __launch_bounds__(256)
k_composite_values_backward(ValuesParams p, const float* __restrict__ gimg, const float* __restrict__ gT, float* __restrict__ dop,
                            float* __restrict__ dval, float* __restrict__ dsc) {
    const int tid = threadIdx.x, lane = tid & 63;
    const ValuesBackwardPix S((int)blockIdx.x, ValuesBackwardPix::nx(p), ValuesBackwardPix::ny(p), p.W, p.H);
    const int b = S.b;
    const int64_t pix = S.pix, list = (int64_t)b * p.K * S.HW + pix;  // (slot k of face [B,K,H,W]: list + k HW)
    __shared__ ValuesLds<KMAX> L;
    for (int i = tid; i < STAB; i += 256) { L.key[i] = STAB_EMPTY; L.val[i][0] = 0.0; L.val[i][1] = 0.0; }
    {
        float T = 1.f;
        for (int k = 0; k < p.K; k++) {
            const int face = S.inside ? p.face[list + k * S.HW] : -1;
            L.tv[k][tid] = T; L.ev[k][tid] = 0.f;
            if ((uint32_t)face < (uint32_t)p.F) T = T * (1.f - p.opacity[face]);
        }
    }
    __syncthreads();
    const bool need_e = dop || dsc;
    if (gimg && S.inside && (need_e || dval)) {  // (no merge and no barrier in here: a lane outside the image skips it)
        for (int c0 = 0; c0 < p.C; c0 += CH) {
            float g[CH];
#pragma unroll
            for (int c = 0; c < CH; c++) g[c] = c0 + c < p.C ? gimg[((int64_t)b * p.C + c0 + c) * S.HW + pix] : 0.f;
            for (int k = 0; k < p.K; k++) {
                const int face = p.face[list + k * S.HW];
                const int64_t at = (((int64_t)b * p.K + k) * p.C + c0) * S.HW + pix;
                float q = 0.f;
                const bool used = (uint32_t)face < (uint32_t)p.F;
                if (used) {
                    const float w = L.tv[k][tid] * p.opacity[face];
                    q = p.scale ? w * p.scale[(int64_t)b * p.F + face] : w;
                    if (need_e && (dop || w != 0.f)) {
                        float e = 0.f;
#pragma unroll
                        for (int c = 0; c < CH; c++)
                            if (c0 + c < p.C) e += p.values[at + (int64_t)c * S.HW] * g[c];
                        L.ev[k][tid] += e;
                    }
                }
                if (dval) {
#pragma unroll
                    for (int c = 0; c < CH; c++)
                        if (c0 + c < p.C) dval[at + (int64_t)c * S.HW] = used ? q * g[c] : 0.f;  // (a literal 0: the upstream may be no number)
                }
            }
        }
    }
    if (!dop && !dsc) return;  // uniform
    float R = (gT && S.inside) ? gT[(int64_t)b * S.HW + pix] : 0.f;
    for (int k = p.K - 1; k >= 0; k--) {
        const int face = S.inside ? p.face[list + k * S.HW] : -1;
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

// the arguments both interpolate calls share -> InterpParams
int interp_params(const char* name, int B, int K, int H, int W, int P, int F, int C, const int32_t* face, const float* bary,
                  const int32_t* faces, const float* vert_attrs, InterpParams& p) {
    return deferred_interp_params(name, DEFER_MAX_C, B, K, H, W, P, F, C, face, bary, faces, vert_attrs, nullptr, 0, (int64_t)K * H * W, p);
}

// the arguments both composite_values calls share -> ValuesParams
int values_params(const char* name, int B, int K, int H, int W, int F, int C, const int32_t* face, const float* faces_opacity,
                  const float* values, const float* face_scale, ValuesParams& p) {
    return deferred_values_params(name, DEFER_MAX_C, B, K, H, W, F, C, face, faces_opacity, values, face_scale, nullptr, 0, (int64_t)K * H * W, p);
}

template <int KMAX>
void launch_values_backward(const ValuesParams& p, hipStream_t st, const float* gi, const float* gt, float* dop, float* dval, float* dsc) {
    const dim3 groups((unsigned)(p.B * ValuesBackwardPix::nx(p) * ValuesBackwardPix::ny(p))), block(256);
    if (p.C <= 4) k_composite_values_backward<KMAX, 4><<<groups, block, 0, st>>>(p, gi, gt, dop, dval, dsc);
    else k_composite_values_backward<KMAX, 8><<<groups, block, 0, st>>>(p, gi, gt, dop, dval, dsc);
}

}  // namespace
}  // namespace dmr

extern "C" {

int dmr_interpolate_fragments(int B, int K, int H, int W, int P, int F, int C, const int32_t* face, const float* bary,
                              const int32_t* faces, const float* vert_attrs, float* out, void* stream) {
    using namespace dmr;
    const char* name = "dmr_interpolate_fragments";
    InterpParams p;
    if (interp_params(name, B, K, H, W, P, F, C, face, bary, faces, vert_attrs, p)) return 1;
    if (!out) return api_fail("dmr_interpolate_fragments: null output");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 rows((unsigned)(B * p.sx * p.sy)), block(256);
    if (C <= 4) k_interpolate_fragments<4><<<rows, block, 0, st>>>(p, out);
    else k_interpolate_fragments<8><<<rows, block, 0, st>>>(p, out);
    return launched(name);
}

int dmr_interpolate_fragments_backward(int B, int K, int H, int W, int P, int F, int C, const int32_t* face, const float* bary,
                                       const int32_t* faces, const float* vert_attrs, const float* grad_out,
                                       float* dL_dvert_attrs, float* dL_dbary, void* stream) {
    using namespace dmr;
    const char* name = "dmr_interpolate_fragments_backward";
    InterpParams p;
    if (interp_params(name, B, K, H, W, P, F, C, face, bary, faces, vert_attrs, p)) return 1;
    if (!grad_out) return api_fail("dmr_interpolate_fragments_backward: null grad_out");
    if (!dL_dvert_attrs && !dL_dbary) return 0;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    zero_on(st, dL_dvert_attrs, (int64_t)P * C, nullptr, 0, nullptr, 0);
    if (launched(name)) return 1;
    const dim3 groups((unsigned)(B * InterpBackwardPix::nx(p) * InterpBackwardPix::ny(p))), block(256);
    if (C <= 4) k_interpolate_fragments_backward<4><<<groups, block, 0, st>>>(p, grad_out, dL_dvert_attrs, dL_dbary);
    else k_interpolate_fragments_backward<8><<<groups, block, 0, st>>>(p, grad_out, dL_dvert_attrs, dL_dbary);
    return launched(name);
}

int dmr_composite_values(int B, int K, int H, int W, int F, int C, const int32_t* face, const float* faces_opacity,
                         const float* values, const float* face_scale, float* image, float* T, void* stream) {
    using namespace dmr;
    const char* name = "dmr_composite_values";
    ValuesParams p;
    if (values_params(name, B, K, H, W, F, C, face, faces_opacity, values, face_scale, p)) return 1;
    if (!image || !T) return api_fail("dmr_composite_values: null output");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 rows((unsigned)(B * p.sx * p.sy)), block(256);
    if (C <= 4) k_composite_values<4><<<rows, block, 0, st>>>(p, image, T);
    else k_composite_values<16><<<rows, block, 0, st>>>(p, image, T);
    return launched(name);
}

int dmr_composite_values_backward(int B, int K, int H, int W, int F, int C, const int32_t* face, const float* faces_opacity,
                                  const float* values, const float* face_scale, const float* grad_image, const float* grad_T,
                                  float* dL_dfaces_opacity, float* dL_dvalues, float* dL_dface_scale, void* stream) {
    using namespace dmr;
    const char* name = "dmr_composite_values_backward";
    ValuesParams p;
    if (values_params(name, B, K, H, W, F, C, face, faces_opacity, values, face_scale, p)) return 1;
    if (dL_dface_scale && !face_scale) return api_fail("dmr_composite_values_backward: dL_dface_scale without face_scale");
    if (!dL_dfaces_opacity && !dL_dvalues && !dL_dface_scale) return 0;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    float *dop, *dval, *dsc;
    const int go = values_backward_prologue(name, st, B, F, (int64_t)B * K * C * H * W, grad_image, grad_T, dL_dfaces_opacity, dL_dvalues,
                                            dL_dface_scale, dop, dval, dsc);
    if (go != SHADE_LAUNCH) return go;
    with_kmax(K, [&](auto kmax) {
        launch_values_backward<decltype(kmax)::value>(p, st, grad_image, grad_T, dop, dval, dsc);
    });
    return launched(name);
}

}  // extern "C"
