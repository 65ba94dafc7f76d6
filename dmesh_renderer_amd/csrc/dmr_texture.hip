// dmr_texture.hip -- shading over per-pixel fragment lists (include/dmesh_renderer_amd_texture.h): bilinear sampling of one
// channel-last texture at per-corner UVs, fused with the compositing, forward and backward.  The model is
// fragments.composite_texture (fragments.py); what is computed, with o_k, T_k, w_k, s_k as in dmr_shade.hip:
//     (s, t)_k = (1 - u - v) UV[c0] + u UV[c1] + v UV[c2],  x = s Wt - 0.5, y = t Ht - 0.5, x0 = floor(x), fx = x - x0 (likewise y),
//     c_k = (1-fy) ((1-fx) tex[iy0,ix0] + fx tex[iy0,ix1]) + fy ((1-fx) tex[iy1,ix0] + fx tex[iy1,ix1]),   ix0 = wrap(x0), ix1 = wrap(x0+1),
//     image = sum_k w_k s_k c_k, T = T_K
// A translation unit of its own, beside dmr_shade.hip: no dmr_scene, no scratch buffer, and no kernel of another unit
// changes.  Both kernels use the fragment kernels' pixel-to-lane mapping (FragSlots, dmr_device.hpp): one 256-thread
// workgroup per 16 x 16 tile, one lane per pixel.
//
// Memory safety does not depend on the input bits: the wrap is done in float, the float is clamped into [-1, n] before it
// becomes an integer, and wrap_pair's last step clamps both indices into [0, n-1]; every load, LDS key and atomic below takes
// its texel from there.  A NaN, an infinity or a UV of 1e30 addresses the texture in bounds (what it computes is unspecified).
//
// None of the arithmetic here decides an index or a branch another kernel depends on: it may contract to FMA.
#include "dmr_shade_common.hpp"
#include "dmr_texture_wrap.hpp"
#include "../../include/dmesh_renderer_amd_texture.h"

namespace dmr {
namespace {

#pragma clang fp contract(fast)

constexpr int TEX_MAX_C = 32;
constexpr int TEX_CHUNKS = TEX_MAX_C / 4;
// The backward's table of texel gradients: keyed by texel x channel chunk, four f64 sums per cell; the scheme and the probe
// bound of dmr_shade_common.hpp at a size of its own (a tile's pixels share a few hundred texels per layer), as large as
// leaves two workgroups per CU their LDS beside the KMAX slots of T_k and e_k (160 KB per CU): 1600 cells at KMAX 4, 1408 at 8,
// 1024 above.
template <int KMAX> constexpr int TTAB = KMAX <= 4 ? 1600 : (KMAX <= 8 ? 1408 : 1024);

struct TexParams {
    int B, K, H, W, Pu, F, C, Ht, Wt, wrap, gx, gy;
    int nch;  // ceil(C / 4): channel chunks per texel
    int vec;  // a texel's chunk may be read as float4 (C % 4 == 0, 16-byte aligned base)
    const int32_t* __restrict__ face;     // [B,K,H,W]
    const float* __restrict__ bary;       // [B,K,2,H,W]
    const int32_t* __restrict__ uvf;      // [F,3]
    const float* __restrict__ opacity;    // [F]
    const float* __restrict__ uvs;        // [Pu,2]
    const float* __restrict__ tex;        // [Ht,Wt,C]
    const float* __restrict__ scale;      // [B,F] or null
};

// wrap_pair(x0, n, wrap, i0, i1): dmr_texture_wrap.hpp.

// A slot's sample: the four texels (row-major indices into [Ht*Wt]: 00 = (iy0, ix0), 01 = (iy0, ix1), 10, 11) and the cell's
// fractions.  (S_j, T_j): the corners' UVs.
struct TexSample {
    uint32_t t[4];
    float fx, fy;
    float S[3], T[3];
};

// The three UV rows of a face; false when one of them is no row of vert_uvs (such a slot samples and scatters nothing).
__device__ __forceinline__ bool uv_corners(const TexParams& p, int face, int (&c)[3]) {
    c[0] = p.uvf[3 * face]; c[1] = p.uvf[3 * face + 1]; c[2] = p.uvf[3 * face + 2];
    return (uint32_t)c[0] < (uint32_t)p.Pu && (uint32_t)c[1] < (uint32_t)p.Pu && (uint32_t)c[2] < (uint32_t)p.Pu;
}

__device__ __forceinline__ void tex_sample(const TexParams& p, const int (&c)[3], float b0, float bu, float bv, TexSample& sm) {
#pragma unroll
    for (int j = 0; j < 3; j++) { sm.S[j] = p.uvs[2 * (int64_t)c[j]]; sm.T[j] = p.uvs[2 * (int64_t)c[j] + 1]; }
    const float s = b0 * sm.S[0] + bu * sm.S[1] + bv * sm.S[2], t = b0 * sm.T[0] + bu * sm.T[1] + bv * sm.T[2];
    const float x = s * (float)p.Wt - 0.5f, y = t * (float)p.Ht - 0.5f;
    const float x0 = floorf(x), y0 = floorf(y);
    sm.fx = x - x0; sm.fy = y - y0;
    int ix0, ix1, iy0, iy1;
    wrap_pair(x0, p.Wt, p.wrap, ix0, ix1);
    wrap_pair(y0, p.Ht, p.wrap, iy0, iy1);
    const uint32_t r0 = (uint32_t)iy0 * (uint32_t)p.Wt, r1 = (uint32_t)iy1 * (uint32_t)p.Wt;
    sm.t[0] = r0 + (uint32_t)ix0; sm.t[1] = r0 + (uint32_t)ix1; sm.t[2] = r1 + (uint32_t)ix0; sm.t[3] = r1 + (uint32_t)ix1;
}

// channels c0 .. c0 + 3 of texel t (0 past C)
__device__ __forceinline__ void load_texel(const TexParams& p, uint32_t t, int c0, float (&r)[4]) {
    const float* __restrict__ row = p.tex + (int64_t)t * p.C + c0;
    if (p.vec) {
        const float4 v = *reinterpret_cast<const float4*>(row);
        r[0] = v.x; r[1] = v.y; r[2] = v.z; r[3] = v.w;
    } else {
#pragma unroll
        for (int c = 0; c < 4; c++) r[c] = c0 + c < p.C ? row[c] : 0.f;
    }
}

// ---------------------------------------------------------------------------
// Forward.  One walk per pixel, every channel's accumulator in registers (NCH = 1: C <= 4; NCH = 8: C <= 32, the chunk loop
// unrolled under uniform guards).  Per slot the (s, t), the four texel indices and the four weights are formed once, then
// the channels run in chunks of four.  A slot of weight 0 -- empty, opacity 0, or behind a face of opacity 1 -- gathers
// nothing.  No LDS, no barrier: lanes outside the image leave at once.
// ---------------------------------------------------------------------------
template <int NCH>
__global__ void __launch_bounds__(256)
k_composite_texture(TexParams p, float* __restrict__ image, float* __restrict__ Tout) {
    const auto [tx, ty, b] = tile_coords((int)blockIdx.x, p.gx, p.gy);
    const FragSlots S(tx, ty, b, p.K, p.W, p.H);
    if (!S.inside) return;
    const int64_t pix = (int64_t)p.W * S.py + S.px;
    float acc[4 * NCH];
#pragma unroll
    for (int c = 0; c < 4 * NCH; c++) acc[c] = 0.f;
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
        int c[3];
        if (!uv_corners(p, face, c)) continue;
        const float q = p.scale ? w * p.scale[(int64_t)b * p.F + face] : w;
        const float bu = p.bary[S.grad_at(k, 0)], bv = p.bary[S.grad_at(k, 1)];
        TexSample sm;
        tex_sample(p, c, 1.f - bu - bv, bu, bv, sm);
        const float wy0 = q * (1.f - sm.fy), wy1 = q * sm.fy;
        const float w00 = wy0 * (1.f - sm.fx), w01 = wy0 * sm.fx, w10 = wy1 * (1.f - sm.fx), w11 = wy1 * sm.fx;
#pragma unroll
        for (int i = 0; i < NCH; i++) {
            if (4 * i >= p.C) break;  // (uniform)
            float r0[4], r1[4], r2[4], r3[4];
            load_texel(p, sm.t[0], 4 * i, r0); load_texel(p, sm.t[1], 4 * i, r1);
            load_texel(p, sm.t[2], 4 * i, r2); load_texel(p, sm.t[3], 4 * i, r3);
#pragma unroll
            for (int j = 0; j < 4; j++) acc[4 * i + j] += w00 * r0[j] + w01 * r1[j] + w10 * r2[j] + w11 * r3[j];
        }
    }
#pragma unroll
    for (int c = 0; c < 4 * NCH; c++)
        if (c < p.C) image[((int64_t)b * p.C + c) * S.HW + pix] = acc[c];
    Tout[(int64_t)b * S.HW + pix] = T;
}

// ---------------------------------------------------------------------------
// Backward.  The structure of k_composite_fragments_backward (dmr_shade.hip), with the merge and the table it shares through
// dmr_shade_common.hpp.  Walk 0, the last walk and the forward's slot head are copies of that unit's text on purpose: DESIGN.md 5c.
//
// LDS: T_k and e_k = c_k . g of every slot of the tile's pixels; the table of UV rows (STAB cells of two f64 sums, re-keyed
// by face for the opacity walk, whose two sums it then holds); and, only in the instantiation that writes dL/dtexture
// (TEX), the texel table: TTAB<KMAX> cells of four f64 sums keyed by texel x channel chunk.  f64 cells as in dmr_shade.hip.
// KMAX 4: 8 KB + 11 KB (+ 56 KB) ... KMAX 32: 64 KB + 11 KB (+ 36 KB).
// ---------------------------------------------------------------------------
template <int KMAX, bool TEX>
struct TexLds {
    float tv[KMAX][TILE_PIX];
    float ev[KMAX][TILE_PIX];
    double uval[STAB][2];
    uint32_t ukey[STAB];
    double tval[TEX ? TTAB<KMAX> : 1][4];
    uint32_t tkey[TEX ? TTAB<KMAX> : 1];
};

// One workgroup per tile, a lane owns its pixel.  With g the pixel's upstream of the image, gT that of T, q_k = w_k s_k:
//   walk 0 (front to back, no gathers): T_k of every slot -> LDS.
//   walk 1 (front to back), per slot: (s, t), the four texels and the cell's fractions once; then per chunk of four channels
//     e_k += c_k . g, dx += (dc/dx) . g, dy += (dc/dy) . g (the gather: only with a reader), and q_k weight g[c] of the four
//     texels into the texel table (a cell the table refuses goes out with direct atomics).  Then Gs = q Wt dx, Gt = q Ht dy,
//     dL/dbary = (u: (S1-S0) Gs + (T1-T0) Gt, v alike) stored by the slot's one lane, and beta_j (Gs, Gt) of the three corners:
//     merged over the wave's lanes of equal face, then into the table keyed by UV row.  Both tables leave once.
//   last walk, back to front: as dmr_shade.hip (d_k = s_k e_k, dL/do_k = T_k (d_k - R_k), R_{k-1} = o_k d_k + (1 - o_k) R_k, exact
//     for opacities 0 and 1; dL/ds_k = w_k e_k), merged by face, into the small table re-keyed by face.
// Slots behind a face of opacity 1 (T_k = 0) gather nothing unless dL/do is wanted.  Every lane of the workgroup runs every
// walk (merges, barriers).
template <int KMAX, bool TEX>
__global__ void __launch_bounds__(256)
k_composite_texture_backward(TexParams p, const float* __restrict__ gimg, const float* __restrict__ gT, float* __restrict__ dop,
                             float* __restrict__ duv, float* __restrict__ dtex, float* __restrict__ dsc, float* __restrict__ dbary) {
    const int tid = threadIdx.x, lane = tid & 63;
    const auto [tx, ty, b] = tile_coords((int)blockIdx.x, p.gx, p.gy);
    const FragSlots S(tx, ty, b, p.K, p.W, p.H);
    const int64_t pix = (int64_t)p.W * S.py + S.px;
    __shared__ TexLds<KMAX, TEX> L;
    for (int i = tid; i < STAB; i += 256) { L.ukey[i] = STAB_EMPTY; L.uval[i][0] = 0.0; L.uval[i][1] = 0.0; }
    if constexpr (TEX)
        for (int i = tid; i < TTAB<KMAX>; i += 256) {
            L.tkey[i] = STAB_EMPTY;
#pragma unroll
            for (int c = 0; c < 4; c++) L.tval[i][c] = 0.0;
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
    if (gimg) {
        const bool need_e = dop || dsc, need_g = duv || dbary;
        float g0[4];
#pragma unroll
        for (int c = 0; c < 4; c++) g0[c] = (S.inside && c < p.C) ? gimg[((int64_t)b * p.C + c) * S.HW + pix] : 0.f;
        for (int k = 0; k < p.K; k++) {
            const int face = S.inside ? p.face[S.face_at(k)] : -1;
            int key = -1, c[3] = {0, 0, 0};
            float du = 0.f, dv = 0.f;
            float rows[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            const float T = L.tv[k][tid];
            // (a slot behind a face of opacity 1, T_k = 0, still has its e_k read by that face's dL/do: what it would uncover)
            if ((uint32_t)face < (uint32_t)p.F && (T != 0.f || dop) && uv_corners(p, face, c)) {
                const float q = T * p.opacity[face] * (p.scale ? p.scale[(int64_t)b * p.F + face] : 1.f);
                const bool gather = need_e || (need_g && q != 0.f), scatter = TEX && q != 0.f;
                if (gather || scatter) {
                    const float bu = p.bary[S.grad_at(k, 0)], bv = p.bary[S.grad_at(k, 1)];
                    const float b0 = 1.f - bu - bv;
                    TexSample sm;
                    tex_sample(p, c, b0, bu, bv, sm);
                    const float ax = 1.f - sm.fx, ay = 1.f - sm.fy;
                    const float wq[4] = {q * ay * ax, q * ay * sm.fx, q * sm.fy * ax, q * sm.fy * sm.fx};
                    float e = 0.f, dx = 0.f, dy = 0.f;
                    for (int c0 = 0, ch = 0; c0 < p.C; c0 += 4, ch++) {
                        float g[4];
#pragma unroll
                        for (int j = 0; j < 4; j++) g[j] = g0[j];
                        if (c0 > 0) {
#pragma unroll
                            for (int j = 0; j < 4; j++) g[j] = c0 + j < p.C ? gimg[((int64_t)b * p.C + c0 + j) * S.HW + pix] : 0.f;
                        }
                        if (gather) {
                            float r0[4], r1[4], r2[4], r3[4];
                            load_texel(p, sm.t[0], c0, r0); load_texel(p, sm.t[1], c0, r1);
                            load_texel(p, sm.t[2], c0, r2); load_texel(p, sm.t[3], c0, r3);
                            float e0 = 0.f, e1 = 0.f, e2 = 0.f, e3 = 0.f;
#pragma unroll
                            for (int j = 0; j < 4; j++) { e0 += r0[j] * g[j]; e1 += r1[j] * g[j]; e2 += r2[j] * g[j]; e3 += r3[j] * g[j]; }
                            e += ay * (ax * e0 + sm.fx * e1) + sm.fy * (ax * e2 + sm.fx * e3);
                            dx += ay * (e1 - e0) + sm.fy * (e3 - e2);
                            dy += ax * (e2 - e0) + sm.fx * (e3 - e1);
                        }
                        if constexpr (TEX) if (scatter) {
#pragma unroll
                            for (int i = 0; i < 4; i++) {
                                if (wq[i] == 0.f) continue;
                                const uint32_t t = sm.t[i];
                                const int slot = stab_find_n<TTAB<KMAX>>(L.tkey, t * (uint32_t)p.nch + (uint32_t)ch);
#pragma unroll
                                for (int j = 0; j < 4; j++) {
                                    if (c0 + j >= p.C) continue;
                                    if (slot >= 0) atomicAdd(&L.tval[slot][j], (double)(wq[i] * g[j]));
                                    else unsafeAtomicAdd(&dtex[(int64_t)t * p.C + c0 + j], wq[i] * g[j]);
                                }
                            }
                        }
                    }
                    if (need_e) L.ev[k][tid] = e;
                    if (need_g && q != 0.f) {
                        const float Gs = q * (float)p.Wt * dx, Gt = q * (float)p.Ht * dy;
                        du = (sm.S[1] - sm.S[0]) * Gs + (sm.T[1] - sm.T[0]) * Gt;
                        dv = (sm.S[2] - sm.S[0]) * Gs + (sm.T[2] - sm.T[0]) * Gt;
                        if (duv && (Gs != 0.f || Gt != 0.f)) {
                            key = face;
                            rows[0] = b0 * Gs; rows[1] = b0 * Gt; rows[2] = bu * Gs; rows[3] = bu * Gt; rows[4] = bv * Gs; rows[5] = bv * Gt;
                        }
                    }
                }
            }
            if (dbary && S.inside) { dbary[S.grad_at(k, 0)] = du; dbary[S.grad_at(k, 1)] = dv; }
            if (!duv || __ballot(key >= 0) == 0ull) continue;  // (wave-uniform)
            shade_merge(lane, key, rows);
            if (key < 0) continue;
            // (lanes of equal face hold equal UV rows: c is the merged rows' too)
#pragma unroll
            for (int j = 0; j < 3; j++) {
                const int slot = stab_find(L.ukey, (uint32_t)c[j]);
                if (slot >= 0) { atomicAdd(&L.uval[slot][0], (double)rows[2 * j]); atomicAdd(&L.uval[slot][1], (double)rows[2 * j + 1]); }
                else { unsafeAtomicAdd(&duv[2 * (int64_t)c[j]], rows[2 * j]); unsafeAtomicAdd(&duv[2 * (int64_t)c[j] + 1], rows[2 * j + 1]); }
            }
        }
        __syncthreads();
        // both tables leave: two lanes per UV row, four per texel cell (a texel's chunk is 16 contiguous bytes)
        if (duv)
            for (int i = tid; i < STAB * 2; i += 256) {
                const uint32_t rid = L.ukey[i >> 1];
                const double x = L.uval[i >> 1][i & 1];
                if (rid != STAB_EMPTY && x != 0.0) unsafeAtomicAdd(&duv[2 * (int64_t)rid + (i & 1)], (float)x);
            }
        if constexpr (TEX)
            for (int i = tid; i < TTAB<KMAX> * 4; i += 256) {
                const uint32_t rid = L.tkey[i >> 2];
                if (rid == STAB_EMPTY) continue;
                const uint32_t t = rid / (uint32_t)p.nch;
                const int c = (int)(rid - t * (uint32_t)p.nch) * 4 + (i & 3);
                const double x = L.tval[i >> 2][i & 3];
                if (c < p.C && x != 0.0) unsafeAtomicAdd(&dtex[(int64_t)t * p.C + c], (float)x);
            }
    }
    if (!dop && !dsc) return;  // uniform
    __syncthreads();
    for (int i = tid; i < STAB; i += 256) { L.ukey[i] = STAB_EMPTY; L.uval[i][0] = 0.0; L.uval[i][1] = 0.0; }
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
        const int slot = stab_find(L.ukey, (uint32_t)face);
        if (slot >= 0) { atomicAdd(&L.uval[slot][0], (double)fg[0]); atomicAdd(&L.uval[slot][1], (double)fg[1]); }
        else {
            if (dop) unsafeAtomicAdd(&dop[face], fg[0]);
            if (dsc) unsafeAtomicAdd(&dsc[(int64_t)b * p.F + face], fg[1]);
        }
    }
    __syncthreads();
    for (int slot = tid; slot < STAB; slot += 256) {
        const uint32_t rid = L.ukey[slot];
        if (rid == STAB_EMPTY) continue;
        if (dop) unsafeAtomicAdd(&dop[rid], (float)L.uval[slot][0]);
        if (dsc) unsafeAtomicAdd(&dsc[(int64_t)b * p.F + rid], (float)L.uval[slot][1]);
    }
}

#pragma clang fp contract(off)

// the arguments both calls share -> TexParams; non-zero with the error set
int tex_params(const char* name, int B, int K, int H, int W, int Pu, int F, int C, int Ht, int Wt, int wrap, const int32_t* face,
               const float* bary, const int32_t* uv_faces, const float* faces_opacity, const float* vert_uvs, const float* texture,
               const float* face_scale, TexParams& p) {
    const std::string n = std::string(name) + ": ";
    if (shade_check_sizes(n, B, K, H, W, Pu, F, C, TEX_MAX_C)) return 1;
    if (Ht < 1 || Wt < 1) return api_fail((n + "the texture must have at least one texel").c_str());
    if (wrap != 0 && wrap != 1) return api_fail((n + "wrap must be 0 (clamp) or 1 (repeat), got " + std::to_string(wrap)).c_str());
    const int64_t nch = (C + 3) / 4, texels = (int64_t)Ht * Wt;
    if (texels >= (int64_t)0xffffffff || texels * nch >= (int64_t)0xffffffff)
        return api_fail((n + "texture too large: Ht * Wt * ceil(C / 4) must be below 2^32 - 1").c_str());
    const char* missing = (F > 0 && Pu > 0 && !vert_uvs) ? "vert_uvs" : (!texture ? "texture" : nullptr);
    if (shade_check_lists(n, "uv_faces", B, K, H, W, F, face, bary, uv_faces, faces_opacity, face_scale, missing, p)) return 1;
    p.Pu = Pu; p.C = C; p.Ht = Ht; p.Wt = Wt; p.wrap = wrap;
    p.nch = (int)nch;
    p.vec = shade_vec(C, texture);
    p.uvf = uv_faces; p.uvs = vert_uvs; p.tex = texture;
    return 0;
}

template <int KMAX>
void launch_backward(const TexParams& p, hipStream_t st, const float* gi, const float* gt, float* dop, float* duv, float* dtex,
                     float* dsc, float* dbary) {
    // (without an image upstream nothing reaches the texture: its zeros are its gradient, and the table is not needed)
    if (dtex && gi) k_composite_texture_backward<KMAX, true><<<dim3((unsigned)(p.B * p.gx * p.gy)), dim3(256), 0, st>>>(p, gi, gt, dop, duv, dtex, dsc, dbary);
    else k_composite_texture_backward<KMAX, false><<<dim3((unsigned)(p.B * p.gx * p.gy)), dim3(256), 0, st>>>(p, gi, gt, dop, duv, nullptr, dsc, dbary);
}

}  // namespace
}  // namespace dmr

extern "C" {

int dmr_composite_texture(int B, int K, int H, int W, int Pu, int F, int C, int Ht, int Wt, int wrap, const int32_t* face,
                          const float* bary, const int32_t* uv_faces, const float* faces_opacity, const float* vert_uvs,
                          const float* texture, const float* face_scale, float* image, float* T, void* stream) {
    using namespace dmr;
    const char* name = "dmr_composite_texture";
    TexParams p;
    if (tex_params(name, B, K, H, W, Pu, F, C, Ht, Wt, wrap, face, bary, uv_faces, faces_opacity, vert_uvs, texture, face_scale, p)) return 1;
    if (!image || !T) return api_fail("dmr_composite_texture: null output");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)(B * p.gx * p.gy)), block(256);
    if (C <= 4) k_composite_texture<1><<<grid, block, 0, st>>>(p, image, T);
    else k_composite_texture<TEX_CHUNKS><<<grid, block, 0, st>>>(p, image, T);
    return launched(name);
}

int dmr_composite_texture_backward(int B, int K, int H, int W, int Pu, int F, int C, int Ht, int Wt, int wrap, const int32_t* face,
                                   const float* bary, const int32_t* uv_faces, const float* faces_opacity, const float* vert_uvs,
                                   const float* texture, const float* face_scale, const float* grad_image, const float* grad_T,
                                   float* dL_dfaces_opacity, float* dL_dvert_uvs, float* dL_dtexture, float* dL_dface_scale,
                                   float* dL_dbary, void* stream) {
    using namespace dmr;
    const char* name = "dmr_composite_texture_backward";
    TexParams p;
    if (tex_params(name, B, K, H, W, Pu, F, C, Ht, Wt, wrap, face, bary, uv_faces, faces_opacity, vert_uvs, texture, face_scale, p)) return 1;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int r = shade_backward_prologue(name, p, grad_image, grad_T, dL_dfaces_opacity, dL_dface_scale, dL_dbary,
                                          {{dL_dvert_uvs, (int64_t)Pu * 2}, {dL_dtexture, (int64_t)Ht * Wt * C}}, st);
    if (r != SHADE_LAUNCH) return r;
    with_kmax(K, [&](auto kmax) {
        launch_backward<decltype(kmax)::value>(p, st, grad_image, grad_T, dL_dfaces_opacity, dL_dvert_uvs, dL_dtexture, dL_dface_scale, dL_dbary);
    });
    return launched(name);
}

}  // extern "C"
