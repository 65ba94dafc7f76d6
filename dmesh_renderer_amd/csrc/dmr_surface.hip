// dmr_surface.hip -- the surface frame of packed rows (include/dmesh_renderer_amd_surface.h): per counting slot the hit point,
// the unit geometric normal of its face turned towards the camera and the mirrored view ray, as three [N,3] row tensors, and
// their gradients to verts, the barycentrics and the camera centres.  The model is fragments.surface_packed:
//     h = (1 - u - v) p0 + u p1 + v p2      g = (p1 - p0) x (p2 - p0), a = |g|, m = g / a (0 when a is not finite or below 1e-20)
//     w = h - origin[b], d = w / |w| (0 when |w| is not finite or below 1e-8)      s = m . d
//     hit = h      normal = m if s <= 0 else -m      reflect = d - 2 s m
// A slot COUNTS when 0 <= row < N and its face id lies in [0, F) (dmr_packed.hip's rule): every access to an [N,3] buffer is behind
// the first test, every read of `faces` behind the second, every read of `verts` behind interp_verts.  Offsets into the [N,3]
// buffers are int64_t.
//
// The forward has k_interpolate_packed's lanes and walk (RowPix: a wave on 64 pixels of an image row, the next slot's face and
// row prefetched) and its plain per-lane stores: three rows of 12 bytes (profiles/packed/store_shapes.txt: the faster shape at
// C <= 8).  h is packed_interp_chunk's expression under the same contraction, so hit is dmr_interpolate_packed's out bit for bit.
// The backward has k_interpolate_packed_backward's tiles (InterpBackwardPix: a workgroup is a tile of ONE view): the nine
// vertex-gradient floats of a slot merge over the wave's lanes of equal face (shade_merge), go into the tile's LDS table keyed
// by vertex (f64 cells; direct atomics when stab_find refuses) and leave once; dL/dbary is a plain store; dL/dorigin sums per
// lane over the slots, per wave by DPP, per workgroup in three f64 LDS cells and leaves as at most three float atomics.  The
// kernel is a template of what is wanted: without dL_dverts there is no merge and no table, with dL_dbary alone no barrier.
#include <cfloat>

#include "dmr_deferred_common.hpp"
#include "dmr_rows_common.hpp"
#include "../../include/dmesh_renderer_amd_surface.h"

namespace dmr {
namespace {

#pragma clang fp contract(fast)

constexpr int SURFACE_TAIL_GROUPS = 32;
constexpr float SURFACE_MIN_AREA = 1e-20f, SURFACE_MIN_LENGTH = 1e-8f;

struct SurfaceParams {
    int B, K, H, W, P, F, C, N, gx, gy, sx, sy;
    const int32_t* __restrict__ face;     // [B,K,H,W]
    const float* __restrict__ bary;       // [B,K,2,H,W]
    const int32_t* __restrict__ row;      // [B,K,H,W]
    const int32_t* __restrict__ n_used;   // [1]
    const int32_t* __restrict__ faces;    // [F,3]
    const float* __restrict__ verts;      // [P,3]
    const float* __restrict__ origin;     // [B,3]
};

// the frame of a counting slot, and what the backward needs of the way to it
struct SurfaceFrame {
    float e1[3], e2[3], h[3], m[3], d[3];
    float inv_a, inv_len, s, b0;  // 1 / a, 1 / len (0 where the rule below gives the zero vector)
    bool face_ok, dir_ok;         // a, len finite and not below their constants
};
__device__ __forceinline__ SurfaceFrame surface_frame(const SurfaceParams& p, const int (&v)[3], float bu, float bv, const float (&o)[3]) {
    SurfaceFrame f;
    float r0[3], r1[3], r2[3];
#pragma unroll
    for (int c = 0; c < 3; c++) { r0[c] = p.verts[(int64_t)v[0] * 3 + c]; r1[c] = p.verts[(int64_t)v[1] * 3 + c]; r2[c] = p.verts[(int64_t)v[2] * 3 + c]; }
    const float b0 = 1.f - bu - bv;
    f.b0 = b0;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        f.h[c] = b0 * r0[c] + bu * r1[c] + bv * r2[c];  // (packed_interp_chunk's expression)
        f.e1[c] = r1[c] - r0[c]; f.e2[c] = r2[c] - r0[c];
    }
    const float gx = f.e1[1] * f.e2[2] - f.e1[2] * f.e2[1], gy = f.e1[2] * f.e2[0] - f.e1[0] * f.e2[2], gz = f.e1[0] * f.e2[1] - f.e1[1] * f.e2[0];
    const float a = sqrtf(gx * gx + gy * gy + gz * gz);
    const bool face_ok = a >= SURFACE_MIN_AREA && a <= FLT_MAX;  // (false for NaN)
    f.face_ok = face_ok;
    f.inv_a = face_ok ? 1.f / a : 0.f;
    f.m[0] = face_ok ? gx * f.inv_a : 0.f; f.m[1] = face_ok ? gy * f.inv_a : 0.f; f.m[2] = face_ok ? gz * f.inv_a : 0.f;
    const float wx = f.h[0] - o[0], wy = f.h[1] - o[1], wz = f.h[2] - o[2];
    const float len = sqrtf(wx * wx + wy * wy + wz * wz);
    const bool dir_ok = len >= SURFACE_MIN_LENGTH && len <= FLT_MAX;
    f.dir_ok = dir_ok;
    f.inv_len = dir_ok ? 1.f / len : 0.f;
    f.d[0] = dir_ok ? wx * f.inv_len : 0.f; f.d[1] = dir_ok ? wy * f.inv_len : 0.f; f.d[2] = dir_ok ? wz * f.inv_len : 0.f;
    f.s = f.m[0] * f.d[0] + f.m[1] * f.d[1] + f.m[2] * f.d[2];
    return f;
}

// rows min(n_used, N) .. N - 1 of the three outputs -> exact zeros: what the SURFACE_TAIL_GROUPS workgroups past the kernel's own do
__device__ __forceinline__ void surface_zero_tail(const SurfaceParams& p, float* __restrict__ a, float* __restrict__ b, float* __restrict__ c, int tail) {
    int u = p.n_used[0];
    u = u < 0 ? 0 : (u > p.N ? p.N : u);
    const int64_t end = (int64_t)p.N * 3;
    for (int64_t i = (int64_t)u * 3 + tail * 256 + (int)threadIdx.x; i < end; i += (int64_t)SURFACE_TAIL_GROUPS * 256) { a[i] = 0.f; b[i] = 0.f; c[i] = 0.f; }
}

// ---------------------------------------------------------------------------
// forward.  One lane per pixel; a slot without a row stores nothing, a slot with a row that is empty for this call (its face id
// outside [0, F), or a vertex that is no row of verts) stores three rows of exact zeros.  No LDS, no barrier.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_surface_packed(SurfaceParams p, int main_groups, float* __restrict__ hit, float* __restrict__ normal, float* __restrict__ reflect) {
    if ((int)blockIdx.x >= main_groups) { surface_zero_tail(p, hit, normal, reflect, (int)blockIdx.x - main_groups); return; }
    const RowPix S((int)blockIdx.x, p.sx, p.sy, p.W, p.H);
    if (!S.inside) return;
    const float o[3] = {p.origin[3 * S.b], p.origin[3 * S.b + 1], p.origin[3 * S.b + 2]};
    int nface = p.face[(int64_t)S.b * p.K * S.HW + S.pix];
    int nrow = p.row[(int64_t)S.b * p.K * S.HW + S.pix];
    for (int k = 0; k < p.K; k++) {
        const int64_t slot = (int64_t)S.b * p.K + k;
        const int face = nface, row = nrow;
        if (k + 1 < p.K) { nface = p.face[(slot + 1) * S.HW + S.pix]; nrow = p.row[(slot + 1) * S.HW + S.pix]; }
        if ((uint32_t)row >= (uint32_t)p.N) continue;
        int v[3] = {0, 0, 0};
        float h[3] = {0.f, 0.f, 0.f}, n[3] = {0.f, 0.f, 0.f}, r[3] = {0.f, 0.f, 0.f};
        if ((uint32_t)face < (uint32_t)p.F && interp_verts(p, face, v)) {
            const float bu = p.bary[(2 * slot) * S.HW + S.pix], bv = p.bary[(2 * slot + 1) * S.HW + S.pix];
            const SurfaceFrame f = surface_frame(p, v, bu, bv, o);
            const float two_s = 2.f * f.s;
#pragma unroll
            for (int c = 0; c < 3; c++) {
                h[c] = f.h[c];
                n[c] = f.s <= 0.f ? f.m[c] : -f.m[c];
                r[c] = f.d[c] - two_s * f.m[c];
            }
        }
        const int64_t at = (int64_t)row * 3;
#pragma unroll
        for (int c = 0; c < 3; c++) { hit[at + c] = h[c]; normal[at + c] = n[c]; reflect[at + c] = r[c]; }
    }
}

// ---------------------------------------------------------------------------
// backward.  One workgroup per tile of one view, a lane owns its pixel (InterpBackwardPix).  WV: dL/dverts (merge, table), WB:
// dL/dbary (a plain store per slot inside the image: an exact 0 where the slot does not count), WO: dL/dorigin.  An upstream
// that is null is zero.  With WV or WO every lane of the workgroup runs every slot, those outside the image with key -1.
// ---------------------------------------------------------------------------
struct SurfaceLds {
    double val[STAB][3];
    uint32_t key[STAB];
};

template <int CTRL>
__device__ __forceinline__ float surface_dpp(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}
// the sum of v over the wave's 64 lanes (called by all 64): quad_perm [1,0,3,2], [2,3,0,1], row_half_mirror, row_mirror give
// every lane its 16-lane row's sum; the four rows' sums are read across
__device__ __forceinline__ float surface_wave_sum(float v) {
    v += surface_dpp<0xB1>(v);
    v += surface_dpp<0x4E>(v);
    v += surface_dpp<0x141>(v);
    v += surface_dpp<0x140>(v);
    const int b = __float_as_int(v);
    return (__int_as_float(__builtin_amdgcn_readlane(b, 0)) + __int_as_float(__builtin_amdgcn_readlane(b, 16))) +
           (__int_as_float(__builtin_amdgcn_readlane(b, 32)) + __int_as_float(__builtin_amdgcn_readlane(b, 48)));
}

template <bool WV, bool WB, bool WO>
__global__ void __launch_bounds__(256)
k_surface_packed_backward(SurfaceParams p, const float* __restrict__ ghit, const float* __restrict__ gnormal, const float* __restrict__ greflect,
                          float* __restrict__ dverts, float* __restrict__ dbary, float* __restrict__ dorigin) {
    const int tid = threadIdx.x, lane = tid & 63;
    const InterpBackwardPix S((int)blockIdx.x, InterpBackwardPix::nx(p), InterpBackwardPix::ny(p), p.W, p.H);
    const int b = S.b;
    const int64_t pix = S.pix;
    __shared__ SurfaceLds L;   // (WV) vertex -> three sums; an instantiation that does not use it has none
    __shared__ double org[3];  // (WO) the workgroup's -sum of dL/dw
    (void)L; (void)org;
    if constexpr (WV) {
        for (int i = tid; i < STAB; i += 256) { L.key[i] = STAB_EMPTY; L.val[i][0] = 0.0; L.val[i][1] = 0.0; L.val[i][2] = 0.0; }
    }
    if constexpr (WO) {
        if (tid < 3) org[tid] = 0.0;
    }
    if constexpr (WV || WO) __syncthreads();
    else if (!S.inside) return;
    const float o[3] = {p.origin[3 * b], p.origin[3 * b + 1], p.origin[3 * b + 2]};
    [[maybe_unused]] float dw_sum[3] = {0.f, 0.f, 0.f};  // (WO) sum over the lane's slots of dL/dw
    for (int k = 0; k < p.K; k++) {
        const int64_t slot_at = ((int64_t)b * p.K + k) * S.HW + pix;                          // of face / row [B,K,H,W]
        const int64_t u_at = (2 * ((int64_t)b * p.K + k)) * S.HW + pix, v_at = u_at + S.HW;  // of bary / dL_dbary [B,K,2,H,W]
        const int face = S.inside ? p.face[slot_at] : -1;
        const int row = S.inside ? p.row[slot_at] : -1;
        int key = -1, v[3] = {0, 0, 0};
        float du = 0.f, dv = 0.f;
        float rows[9];
#pragma unroll
        for (int c = 0; c < 9; c++) rows[c] = 0.f;
        if ((uint32_t)row < (uint32_t)p.N && (uint32_t)face < (uint32_t)p.F && interp_verts(p, face, v)) {
            const int64_t at = (int64_t)row * 3;
            float gh[3] = {0.f, 0.f, 0.f}, gn[3] = {0.f, 0.f, 0.f}, gr[3] = {0.f, 0.f, 0.f};
#pragma unroll
            for (int c = 0; c < 3; c++) {
                if (ghit) gh[c] = ghit[at + c];
                if (gnormal) gn[c] = gnormal[at + c];
                if (greflect) gr[c] = greflect[at + c];
            }
            const float bu = p.bary[u_at], bv = p.bary[v_at];
            const SurfaceFrame f = surface_frame(p, v, bu, bv, o);
            const float sigma = f.s <= 0.f ? 1.f : -1.f;
            const float mgr = f.m[0] * gr[0] + f.m[1] * gr[1] + f.m[2] * gr[2];
            float dm[3], dd[3];
#pragma unroll
            for (int c = 0; c < 3; c++) {
                dm[c] = sigma * gn[c] - 2.f * f.s * gr[c] - 2.f * mgr * f.d[c];
                dd[c] = gr[c] - 2.f * mgr * f.m[c];
            }
            const float mdm = f.m[0] * dm[0] + f.m[1] * dm[1] + f.m[2] * dm[2];
            const float ddd = f.d[0] * dd[0] + f.d[1] * dd[1] + f.d[2] * dd[2];
            float dg[3], dh[3];
#pragma unroll
            for (int c = 0; c < 3; c++) {
                dg[c] = f.face_ok ? (dm[c] - f.m[c] * mdm) * f.inv_a : 0.f;      // (selects: an exact 0 whatever the upstreams hold)
                const float dw = f.dir_ok ? (dd[c] - f.d[c] * ddd) * f.inv_len : 0.f;
                dh[c] = gh[c] + dw;
                if constexpr (WO) dw_sum[c] += dw;
            }
            if constexpr (WB) {
                du = f.e1[0] * dh[0] + f.e1[1] * dh[1] + f.e1[2] * dh[2];
                dv = f.e2[0] * dh[0] + f.e2[1] * dh[1] + f.e2[2] * dh[2];
            }
            if constexpr (WV) {
                const float de1[3] = {f.e2[1] * dg[2] - f.e2[2] * dg[1], f.e2[2] * dg[0] - f.e2[0] * dg[2], f.e2[0] * dg[1] - f.e2[1] * dg[0]};
                const float de2[3] = {dg[1] * f.e1[2] - dg[2] * f.e1[1], dg[2] * f.e1[0] - dg[0] * f.e1[2], dg[0] * f.e1[1] - dg[1] * f.e1[0]};
                key = face;
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    rows[c] = f.b0 * dh[c] - de1[c] - de2[c];
                    rows[3 + c] = bu * dh[c] + de1[c];
                    rows[6 + c] = bv * dh[c] + de2[c];
                }
            }
        }
        if constexpr (WB) {
            if (S.inside) { dbary[u_at] = du; dbary[v_at] = dv; }
        }
        if constexpr (WV) {
            if (__ballot(key >= 0) == 0ull) continue;  // (wave-uniform)
            shade_merge(lane, key, rows);
            if (key < 0) continue;
            // (lanes of equal face hold equal vertices: v is the merged rows' too)
#pragma unroll
            for (int j = 0; j < 3; j++) {
                const int slot = stab_find(L.key, (uint32_t)v[j]);
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    if (slot >= 0) atomicAdd(&L.val[slot][c], (double)rows[3 * j + c]);
                    else unsafeAtomicAdd(&dverts[(int64_t)v[j] * 3 + c], rows[3 * j + c]);
                }
            }
        }
    }
    if constexpr (WO) {  // (every lane of the wave is here: those outside the image and without a counting slot add 0)
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float s = surface_wave_sum(dw_sum[c]);
            if (lane == 0 && s != 0.f) atomicAdd(&org[c], -(double)s);
        }
    }
    if constexpr (WV || WO) __syncthreads();
    if constexpr (WV) {
        for (int i = tid; i < STAB * 3; i += 256) {
            const int slot = i / 3, c = i % 3;
            const uint32_t rid = L.key[slot];
            const double x = L.val[slot][c];
            if (rid != STAB_EMPTY && x != 0.0) unsafeAtomicAdd(&dverts[(int64_t)rid * 3 + c], (float)x);
        }
    }
    if constexpr (WO) {
        if (tid < 3 && org[tid] != 0.0) unsafeAtomicAdd(&dorigin[3 * b + tid], (float)org[tid]);
    }
}

#pragma clang fp contract(off)

// what both calls check first, in the header's order -> SurfaceParams
int surface_params(const char* name, int B, int K, int H, int W, int P, int F, int N, const int32_t* face, const float* bary, const int32_t* row,
                   const int32_t* n_used, const int32_t* faces, const float* verts, const float* origin, SurfaceParams& p) {
    const std::string n = std::string(name) + ": ";
    if (shade_check_sizes(n, B, K, H, W, P, F, 3, 3)) return 1;
    if (N < 0) return api_fail((n + "bad rows").c_str());
    if (!face || !bary || !row) return api_fail((n + "null fragment lists").c_str());
    if (F > 0 && !faces) return api_fail((n + "null faces").c_str());
    if ((F > 0 && P > 0 && !verts) || !origin) return api_fail((n + "null verts / origin").c_str());
    if (!n_used) return api_fail((n + "null n_used").c_str());
    if (deferred_grids(n, B, K, H, W, F, 3, SURFACE_TAIL_GROUPS, (int64_t)B * K * H * W, p)) return 1;
    p.P = P; p.N = N;
    p.face = face; p.bary = bary; p.row = row; p.n_used = n_used; p.faces = faces; p.verts = verts; p.origin = origin;
    return 0;
}

// the instantiation of the three wanted outputs (at least one of them)
template <bool WV, bool WB, bool WO>
void launch_surface_backward(const SurfaceParams& p, hipStream_t st, const float* gh, const float* gn, const float* gr, float* dv, float* db, float* dorg) {
    const dim3 groups((unsigned)(p.B * InterpBackwardPix::nx(p) * InterpBackwardPix::ny(p))), block(256);
    k_surface_packed_backward<WV, WB, WO><<<groups, block, 0, st>>>(p, gh, gn, gr, dv, db, dorg);
}

}  // namespace
}  // namespace dmr

extern "C" {

int dmr_surface_packed(int B, int K, int H, int W, int P, int F, int N, const int32_t* face, const float* bary, const int32_t* row,
                       const int32_t* n_used, const int32_t* faces, const float* verts, const float* origin, float* hit,
                       float* normal, float* reflect, void* stream) {
    using namespace dmr;
    const char* name = "dmr_surface_packed";
    SurfaceParams p;
    if (surface_params(name, B, K, H, W, P, F, N, face, bary, row, n_used, faces, verts, origin, p)) return 1;
    if (N == 0) return 0;
    if (!hit || !normal || !reflect) return api_fail("dmr_surface_packed: null output");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int main_groups = B * p.sx * p.sy;
    k_surface_packed<<<dim3((unsigned)(main_groups + SURFACE_TAIL_GROUPS)), dim3(256), 0, st>>>(p, main_groups, hit, normal, reflect);
    return launched(name);
}

int dmr_surface_packed_backward(int B, int K, int H, int W, int P, int F, int N, const int32_t* face, const float* bary,
                                const int32_t* row, const int32_t* n_used, const int32_t* faces, const float* verts,
                                const float* origin, const float* grad_hit, const float* grad_normal, const float* grad_reflect,
                                float* dL_dverts, float* dL_dbary, float* dL_dorigin, void* stream) {
    using namespace dmr;
    const char* name = "dmr_surface_packed_backward";
    SurfaceParams p;
    if (surface_params(name, B, K, H, W, P, F, N, face, bary, row, n_used, faces, verts, origin, p)) return 1;
    if (N > 0 && !grad_hit && !grad_normal && !grad_reflect) return api_fail("dmr_surface_packed_backward: null upstreams");
    if (P == 0) dL_dverts = nullptr;  // (no row to write)
    if (!dL_dverts && !dL_dbary && !dL_dorigin) return 0;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (dL_dverts) {
        rows_fill_on(st, dL_dverts, (int64_t)3 * P, 0u);
        if (launched(name)) return 1;
    }
    if (dL_dorigin) {
        rows_fill_on(st, dL_dorigin, (int64_t)3 * B, 0u);
        if (launched(name)) return 1;
    }
    // (N == 0: no slot counts; the kernel then stores the zeros of dL_dbary, reads no upstream and adds nothing)
    float* const dv = N > 0 ? dL_dverts : nullptr;
    float* const dorg = N > 0 ? dL_dorigin : nullptr;
    if (!dv && !dL_dbary && !dorg) return 0;
    const bool wb = dL_dbary != nullptr;
    if (dv && dorg) { if (wb) launch_surface_backward<true, true, true>(p, st, grad_hit, grad_normal, grad_reflect, dv, dL_dbary, dorg);
                      else launch_surface_backward<true, false, true>(p, st, grad_hit, grad_normal, grad_reflect, dv, dL_dbary, dorg); }
    else if (dv) { if (wb) launch_surface_backward<true, true, false>(p, st, grad_hit, grad_normal, grad_reflect, dv, dL_dbary, dorg);
                   else launch_surface_backward<true, false, false>(p, st, grad_hit, grad_normal, grad_reflect, dv, dL_dbary, dorg); }
    else if (dorg) { if (wb) launch_surface_backward<false, true, true>(p, st, grad_hit, grad_normal, grad_reflect, dv, dL_dbary, dorg);
                     else launch_surface_backward<false, false, true>(p, st, grad_hit, grad_normal, grad_reflect, dv, dL_dbary, dorg); }
    else launch_surface_backward<false, true, false>(p, st, grad_hit, grad_normal, grad_reflect, dv, dL_dbary, dorg);
    return launched(name);
}

}  // extern "C"
