// dmr_packed.hip -- deferred shading over per-pixel fragment lists on PACKED, channel-last rows
// (include/dmesh_renderer_amd_packed.h): dmr_interp.hip's two ends of a deferred shader, with the per-slot tensor [B,K,C,H,W]
// replaced by [N,C] rows, one per used slot.  The models are fragments.pack_slots, interpolate_packed and composite_values_packed:
//     pack:         row[slot] = the number of used slots before `slot` in the flattened [B,K,H,W] lists, -1 in an empty slot and
//                   in a used one past the capacity; n_used = the number of used slots
//     interpolate:  out[row_k, c] = (1 - u - v) A[v0][c] + u A[v1][c] + v A[v2][c]; tail rows zero
//     composite:    image[b,c] = sum_k w_k s_k values[row_k, c], T = T_K, with dmr_interp.hip's o_k, T_k, w_k, s_k
// A slot COUNTS when 0 <= row < N and its face id lies in [0, F): every access to an [N,C] buffer is behind the first test, so
// a `row` made for other lists' sizes stays in bounds.  Offsets into the [N,C] buffers are int64_t.
//
// The lane mappings, the backward kernels' LDS tables, the vertex lookup, the zeroing kernel and the host checks are
// dmr_interp.hip's, stated once for both in dmr_deferred_common.hpp; the walks are this unit's own text.  A wave
// of the forwards sits on 64 pixels of one image
// row at one k, which are 64 consecutive slots of the flattened lists -- its rows are one contiguous range, and its cnt * C
// output floats too.  The arithmetic of a slot is dmr_interp.hip's expression for expression, under the same contraction, so
// the forwards give the dense unit's numbers bit for bit.
#include "dmr_deferred_common.hpp"
#include "../../include/dmesh_renderer_amd_packed.h"

namespace dmr {
namespace {

#pragma clang fp contract(fast)

constexpr int PACKED_MAX_C = 256;

struct PackedInterpParams {
    int B, K, H, W, P, F, C, N, gx, gy, sx, sy;
    int vec;   // rows of vert_attrs may be read as float4 (C % 4 == 0, 16-byte aligned base)
    int rvec;  // ... and rows of out / grad_out
    const int32_t* __restrict__ face;     // [B,K,H,W]
    const float* __restrict__ bary;       // [B,K,2,H,W]
    const int32_t* __restrict__ row;      // [B,K,H,W]
    const int32_t* __restrict__ n_used;   // [1]
    const int32_t* __restrict__ faces;    // [F,3]
    const float* __restrict__ attrs;      // [P,C]
};

struct PackedValuesParams {
    int B, K, H, W, F, C, N, gx, gy, sx, sy;
    int rvec;  // rows of values (and of dL/dvalues) may be accessed as float4
    const int32_t* __restrict__ face;     // [B,K,H,W]
    const int32_t* __restrict__ row;      // [B,K,H,W]
    const int32_t* __restrict__ n_used;   // [1]
    const float* __restrict__ opacity;    // [F]
    const float* __restrict__ values;     // [N,C]
    const float* __restrict__ scale;      // [B,F] or null
};

// channels c0 .. c0 + CH - 1 of a row of C floats that starts at `row` (0 past C)
template <int CH>
__device__ __forceinline__ void packed_load(const float* __restrict__ row, int C, int c0, int vec, float (&r)[CH]) {
    static_assert(CH % 4 == 0, "whole float4");
    if (vec) {
#pragma unroll
        for (int i = 0; i < CH / 4; i++) {
            float4 t = {0.f, 0.f, 0.f, 0.f};
            if (c0 + 4 * i < C) t = *reinterpret_cast<const float4*>(row + c0 + 4 * i);
            r[4 * i] = t.x; r[4 * i + 1] = t.y; r[4 * i + 2] = t.z; r[4 * i + 3] = t.w;
        }
    } else {
#pragma unroll
        for (int c = 0; c < CH; c++) r[c] = c0 + c < C ? row[c0 + c] : 0.f;
    }
}
// ... stored
template <int CH>
__device__ __forceinline__ void packed_store(float* __restrict__ row, int C, int c0, int vec, const float (&r)[CH]) {
    static_assert(CH % 4 == 0, "whole float4");
    if (vec) {
#pragma unroll
        for (int i = 0; i < CH / 4; i++)
            if (c0 + 4 * i < C) *reinterpret_cast<float4*>(row + c0 + 4 * i) = make_float4(r[4 * i], r[4 * i + 1], r[4 * i + 2], r[4 * i + 3]);
    } else {
#pragma unroll
        for (int c = 0; c < CH; c++)
            if (c0 + c < C) row[c0 + c] = r[c];
    }
}

// Rows min(n_used, N) .. N - 1 of an [N,C] buffer -> exact zeros: what TAIL_GROUPS workgroups past a kernel's own do (tail:
// the workgroup's index among them).  The count is read on the device: no host wait, and a replayed graph follows it.
constexpr int TAIL_GROUPS = 32;
__device__ __forceinline__ void packed_zero_tail(const int32_t* __restrict__ n_used, int N, int C, float* __restrict__ buf, int tail) {
    int u = n_used[0];
    u = u < 0 ? 0 : (u > N ? N : u);
    const int64_t end = (int64_t)N * C;
    for (int64_t i = (int64_t)u * C + tail * 256 + (int)threadIdx.x; i < end; i += (int64_t)TAIL_GROUPS * 256) buf[i] = 0.f;
}

// ---------------------------------------------------------------------------
// pack.  Three stream-ordered launches over the lists as one array of n = B K H W ids, PACK_SLOTS of them per workgroup, in
// PACK_PASSES passes of 256 consecutive ids (so that the rows follow the array's order):
//   k_pack_count  the workgroup's number of used slots (ballot + popcount) -> row[first slot of the workgroup]
//   k_pack_scan   ONE workgroup turns those counts into exclusive offsets, in place, PACK_SCAN at a time, and writes n_used
//   k_pack_write  every workgroup reads its offset, then writes the row of each of its slots (-1: empty, or at / past capacity)
// `row` is its own scratch: a workgroup's count and offset sit in the first of its slots, which its k_pack_write overwrites
// after reading it.  No workgroup waits for another inside a kernel.
// ---------------------------------------------------------------------------
constexpr int PACK_PASSES = 8, PACK_SLOTS = 256 * PACK_PASSES, PACK_SCAN = 256;

__global__ void __launch_bounds__(256)
k_pack_count(const int32_t* __restrict__ face, int64_t n, int F, int32_t* __restrict__ row) {
    const int tid = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * PACK_SLOTS;
    __shared__ int wave_count[4];
    int cnt = 0;  // (wave-uniform)
#pragma unroll
    for (int j = 0; j < PACK_PASSES; j++) {
        const int64_t i = base + j * 256 + tid;
        const bool used = i < n && (uint32_t)face[i] < (uint32_t)F;
        cnt += __popcll(__ballot(used));
    }
    if ((tid & 63) == 0) wave_count[tid >> 6] = cnt;
    __syncthreads();
    if (tid == 0) row[base] = wave_count[0] + wave_count[1] + wave_count[2] + wave_count[3];
}

__global__ void __launch_bounds__(PACK_SCAN)
k_pack_scan(int32_t* __restrict__ row, int groups, int32_t* __restrict__ n_used) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    __shared__ int wave_total[PACK_SCAN / 64];
    int carry = 0;  // the used slots of the workgroups before g0 (uniform)
    for (int g0 = 0; g0 < groups; g0 += PACK_SCAN) {
        const int g = g0 + tid;
        const int c = g < groups ? row[(int64_t)g * PACK_SLOTS] : 0;
        int incl = c;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_up(incl, d);
            if (lane >= d) incl += o;
        }
        if (lane == 63) wave_total[wave] = incl;
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int i = 0; i < PACK_SCAN / 64; i++) { before += i < wave ? wave_total[i] : 0; total += wave_total[i]; }
        if (g < groups) row[(int64_t)g * PACK_SLOTS] = carry + before + incl - c;
        carry += total;
        __syncthreads();
    }
    if (tid == 0) n_used[0] = carry;
}

__global__ void __launch_bounds__(256)
k_pack_write(const int32_t* __restrict__ face, int64_t n, int F, int capacity, int32_t* __restrict__ row) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t base = (int64_t)blockIdx.x * PACK_SLOTS;
    __shared__ int wave_count[PACK_PASSES][4];
    __shared__ int first;
    if (tid == 0) first = row[base];
    int below[PACK_PASSES];  // the used slots of the lane's wave before the lane, per pass; -1: the lane's slot is not used
#pragma unroll
    for (int j = 0; j < PACK_PASSES; j++) {
        const int64_t i = base + j * 256 + tid;
        const bool used = i < n && (uint32_t)face[i] < (uint32_t)F;
        const uint64_t m = __ballot(used);
        below[j] = used ? __popcll(m & ((1ull << lane) - 1ull)) : -1;
        if (lane == 0) wave_count[j][wave] = __popcll(m);
    }
    __syncthreads();  // (the offset is read, the counts are in: from here on row is written)
    int run = first;
#pragma unroll
    for (int j = 0; j < PACK_PASSES; j++) {
        int mine = run;
#pragma unroll
        for (int w = 0; w < 4; w++) { mine += w < wave ? wave_count[j][w] : 0; run += wave_count[j][w]; }
        const int64_t i = base + j * 256 + tid;
        const int r = mine + below[j];
        if (i < n) row[i] = (below[j] >= 0 && r < capacity) ? r : -1;
    }
}

// ---------------------------------------------------------------------------
// interpolate, forward.  One lane per pixel (RowPix), k_interpolate_fragments' walk; a slot without a row stores nothing; a
// slot with a row that is empty for this call (its face id outside [0, F), or a vertex that is no row of vert_attrs) stores
// exact zeros.  The TAIL_GROUPS workgroups past main_groups zero the tail rows.  Two store shapes, each used where it measured
// faster (profiles/packed/store_shapes.txt; the ablation build's DMR_ABLATE bit 32768 runs the other one):
//   plain     a slot with a row stores its C floats at out + row C, channel chunk by chunk: every lane its own run of
//             consecutive addresses (float4 where the rows allow it), the wave's runs back to back.  No LDS.  C <= PLAIN_MAX_C,
//             where a row is ONE chunk, and C > STAGE_MAX_C.
//   VIA_LDS   the wave's rows go to LDS chunk by chunk and leave transposed once they are whole, so that consecutive LANES
//             store consecutive addresses: cnt C floats in one contiguous range -- when the rows of the wave's lanes ARE one
//             contiguous range (they are when `row` comes from dmr_pack_slots); a wave whose rows are not takes the plain
//             stores.  No workgroup barrier: a wave reads back what it wrote itself.  PLAIN_MAX_C < C <= STAGE_MAX_C.
// ---------------------------------------------------------------------------
constexpr int PLAIN_MAX_C = 8, STAGE_MAX_C = 32, STAGE_ROW = STAGE_MAX_C + 1;  // (an odd row pitch: a wave's lanes on distinct banks)

// channels c0 .. c0 + CH - 1 of a slot's interpolated attributes (zeros when the slot is empty for this call)
template <int CH>
__device__ __forceinline__ void packed_interp_chunk(const PackedInterpParams& p, bool used, const int (&v)[3], float b0, float bu, float bv,
                                                    int c0, float (&a)[CH]) {
#pragma unroll
    for (int c = 0; c < CH; c++) a[c] = 0.f;
    if (used) {
        float r0[CH], r1[CH], r2[CH];
        packed_load<CH>(p.attrs + (int64_t)v[0] * p.C, p.C, c0, p.vec, r0);
        packed_load<CH>(p.attrs + (int64_t)v[1] * p.C, p.C, c0, p.vec, r1);
        packed_load<CH>(p.attrs + (int64_t)v[2] * p.C, p.C, c0, p.vec, r2);
#pragma unroll
        for (int c = 0; c < CH; c++) a[c] = b0 * r0[c] + bu * r1[c] + bv * r2[c];
    }
}

template <int CH, bool VIA_LDS>
__global__ void __launch_bounds__(256)
k_interpolate_packed(PackedInterpParams p, int main_groups, float* __restrict__ out) {
    if ((int)blockIdx.x >= main_groups) { packed_zero_tail(p.n_used, p.N, p.C, out, (int)blockIdx.x - main_groups); return; }
    const RowPix S((int)blockIdx.x, p.sx, p.sy, p.W, p.H);
    [[maybe_unused]] float* stage = nullptr;  // the wave's 64 rows of C floats
    if constexpr (VIA_LDS) {  // (every lane of the wave stays for the transposed stores: one outside the image has no row)
        __shared__ float lds[4 * 64 * STAGE_ROW];
        stage = lds + (threadIdx.x >> 6) * (64 * STAGE_ROW);
    } else {
        if (!S.inside) return;
    }
    int nface = S.inside ? p.face[(int64_t)S.b * p.K * S.HW + S.pix] : -1;
    int nrow = S.inside ? p.row[(int64_t)S.b * p.K * S.HW + S.pix] : -1;
    for (int k = 0; k < p.K; k++) {
        const int64_t slot = (int64_t)S.b * p.K + k;
        const int face = nface, row = nrow;
        if (k + 1 < p.K && S.inside) { nface = p.face[(slot + 1) * S.HW + S.pix]; nrow = p.row[(slot + 1) * S.HW + S.pix]; }
        const bool has = (uint32_t)row < (uint32_t)p.N;
        if constexpr (!VIA_LDS) {
            if (!has) continue;
        }
        int v[3] = {0, 0, 0};
        const bool used = has && (uint32_t)face < (uint32_t)p.F && interp_verts(p, face, v);
        float bu = 0.f, bv = 0.f;
        if (used) { bu = p.bary[(2 * slot) * S.HW + S.pix]; bv = p.bary[(2 * slot + 1) * S.HW + S.pix]; }
        const float b0 = 1.f - bu - bv;
        if constexpr (VIA_LDS) {
            const int lane = threadIdx.x & 63;
            const uint64_t m = __ballot(has);
            if (m == 0ull) continue;  // (wave-uniform)
            const int rank = __popcll(m & ((1ull << lane) - 1ull));
            const int first = __shfl(row, __ffsll((unsigned long long)m) - 1);
            if (__ballot(has && row != first + rank) == 0ull) {  // (wave-uniform) one contiguous range of rows
                const int pitch = p.C | 1;
                for (int c0 = 0; c0 < p.C; c0 += CH) {
                    float a[CH];
                    packed_interp_chunk<CH>(p, used, v, b0, bu, bv, c0, a);
                    if (has) {
#pragma unroll
                        for (int c = 0; c < CH; c++)
                            if (c0 + c < p.C) stage[rank * pitch + c0 + c] = a[c];
                    }
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
                const uint32_t total = (uint32_t)__popcll(m) * (uint32_t)p.C, inv = ((1u << 20) + (uint32_t)p.C - 1u) / (uint32_t)p.C;
                float* __restrict__ o = out + (int64_t)first * p.C;
                for (uint32_t i = (uint32_t)lane; i < total; i += 64u) {
                    const uint32_t r = (i * inv) >> 20, c = i - r * (uint32_t)p.C;  // (i / C, i % C: exact below 2^20 / C)
                    o[i] = stage[r * (uint32_t)pitch + c];
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
                continue;
            }
            if (!has) continue;
        }
        float* __restrict__ o = out + (int64_t)row * p.C;
        for (int c0 = 0; c0 < p.C; c0 += CH) {
            float a[CH];
            packed_interp_chunk<CH>(p, used, v, b0, bu, bv, c0, a);
            packed_store<CH>(o, p.C, c0, p.rvec, a);
        }
    }
}

// ---------------------------------------------------------------------------
// interpolate, backward: k_interpolate_fragments_backward with g_k read from the slot's row of grad_out, on its table (InterpLds).
// ---------------------------------------------------------------------------
// One workgroup per tile, a lane owns its pixel (InterpBackwardPix).  Per chunk of CH channels, front to back, with g_k
// the upstream's row of the slot: dL/dbary = ((A[v1] - A[v0]) . g_k, (A[v2] - A[v0]) . g_k) (the lane is the slot's one
// writer: the first chunk stores -- an exact 0 in slots that do not count, so nothing is zeroed beforehand -- later ones
// add), and the rows beta_j g_k of the three vertices: merged over the wave's lanes of equal face, then into the table keyed
// by vertex, which leaves once per chunk (its keys stay).  dattr / dbary null: not wanted, and its part is skipped.  With dattr
// every lane of the workgroup runs every slot (merges, barriers): those outside the image with key -1.
template <int CH>
__global__ void __launch_bounds__(256)
k_interpolate_packed_backward(PackedInterpParams p, const float* __restrict__ gout, float* __restrict__ dattr, float* __restrict__ dbary) {
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
            const int64_t slot_at = ((int64_t)b * p.K + k) * S.HW + pix;           // of face / row [B,K,H,W]
            const int64_t u_at = (2 * ((int64_t)b * p.K + k)) * S.HW + pix, v_at = u_at + S.HW;  // of bary / dL_dbary [B,K,2,H,W]
            const int face = S.inside ? p.face[slot_at] : -1;
            const int row = S.inside ? p.row[slot_at] : -1;
            int key = -1, v[3] = {0, 0, 0};
            float du = 0.f, dv = 0.f;
            float rows[3 * CH];
#pragma unroll
            for (int c = 0; c < 3 * CH; c++) rows[c] = 0.f;
            if ((uint32_t)row < (uint32_t)p.N && (uint32_t)face < (uint32_t)p.F && interp_verts(p, face, v)) {
                float g[CH];
                packed_load<CH>(gout + (int64_t)row * p.C, p.C, c0, p.rvec, g);
                if (dbary) {
                    float r0[CH], r1[CH], r2[CH];
                    packed_load<CH>(p.attrs + (int64_t)v[0] * p.C, p.C, c0, p.vec, r0);
                    packed_load<CH>(p.attrs + (int64_t)v[1] * p.C, p.C, c0, p.vec, r1);
                    packed_load<CH>(p.attrs + (int64_t)v[2] * p.C, p.C, c0, p.vec, r2);
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
// composite_values, forward: k_composite_values' walk, a slot's CH values one run of its row (C <= 4: one walk with CH = 4;
// else CH = 16).  A slot that does not count and a slot of weight 0 load nothing.  No LDS, no barrier.
// ---------------------------------------------------------------------------
template <int CH>
__global__ void __launch_bounds__(256)
k_composite_values_packed(PackedValuesParams p, float* __restrict__ image, float* __restrict__ Tout) {
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
            const int row = p.row[(list + k) * S.HW + S.pix];
            if ((uint32_t)row >= (uint32_t)p.N) continue;
            const float o = p.opacity[face];
            const float w = T * o;
            T = T * (1.f - o);
            if (w == 0.f) continue;
            const float q = p.scale ? w * p.scale[(int64_t)S.b * p.F + face] : w;
            float vk[CH];
            packed_load<CH>(p.values + (int64_t)row * p.C, p.C, c0, p.rvec, vk);
#pragma unroll
            for (int c = 0; c < CH; c++)
                if (c0 + c < p.C) acc[c] += q * vk[c];
        }
#pragma unroll
        for (int c = 0; c < CH; c++)
            if (c0 + c < p.C) image[((int64_t)S.b * p.C + c0 + c) * S.HW + S.pix] = acc[c];
        if (c0 == 0) Tout[(int64_t)S.b * S.HW + S.pix] = T;
    }
}

// ---------------------------------------------------------------------------
// composite_values, backward, on k_composite_values_backward's LDS (ValuesLds).
// ---------------------------------------------------------------------------
// One workgroup per 64 x 4 pixels, a lane owns its pixel (ValuesBackwardPix): k_composite_values_backward's three walks.
//   walk 0 (front to back, no values): T_k of every slot -> LDS.
//   per chunk of CH channels, front to back: dL/dvalues[row_k, c] = w_k s_k g[c], a plain store to the row of every slot that
//     has one (a literal 0 where the slot is empty for this call), and e_k += values[row_k] . g (LDS) when dL/do or dL/ds is wanted.
//   last walk, back to front: d_k = s_k e_k, dL/do_k = T_k (d_k - R_k), R_{K-1} = gT, R_{k-1} = o_k d_k + (1 - o_k) R_k (exact
//     for opacities 0 and 1: nothing divides by 1 - o), dL/ds_k = w_k e_k; merged by face, into the table, which leaves once.
// gimg null: no value is read (the host has zeroed dL/dvalues, and passes dval null).  dop / dval / dsc null: not wanted.
// With dval, the TAIL_GROUPS workgroups past main_groups zero the tail rows of dL/dvalues.
template <int KMAX, int CH>
__global__ void __launch_bounds__(256)
k_composite_values_packed_backward(PackedValuesParams p, int main_groups, const float* __restrict__ gimg, const float* __restrict__ gT,
                                   float* __restrict__ dop, float* __restrict__ dval, float* __restrict__ dsc) {
    if ((int)blockIdx.x >= main_groups) { packed_zero_tail(p.n_used, p.N, p.C, dval, (int)blockIdx.x - main_groups); return; }
    const int tid = threadIdx.x, lane = tid & 63;
    const ValuesBackwardPix S((int)blockIdx.x, ValuesBackwardPix::nx(p), ValuesBackwardPix::ny(p), p.W, p.H);
    const int b = S.b;
    const int64_t pix = S.pix, list = (int64_t)b * p.K * S.HW + pix;  // (slot k of face / row [B,K,H,W]: list + k HW)
    __shared__ ValuesLds<KMAX> L;
    for (int i = tid; i < STAB; i += 256) { L.key[i] = STAB_EMPTY; L.val[i][0] = 0.0; L.val[i][1] = 0.0; }
    {
        float T = 1.f;
        for (int k = 0; k < p.K; k++) {
            const int face = S.inside ? p.face[list + k * S.HW] : -1;
            const int row = S.inside ? p.row[list + k * S.HW] : -1;
            L.tv[k][tid] = T; L.ev[k][tid] = 0.f;
            if ((uint32_t)face < (uint32_t)p.F && (uint32_t)row < (uint32_t)p.N) T = T * (1.f - p.opacity[face]);
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
                const int row = p.row[list + k * S.HW];
                if ((uint32_t)row >= (uint32_t)p.N) continue;
                const int face = p.face[list + k * S.HW];
                const int64_t at = (int64_t)row * p.C;
                float q = 0.f;
                const bool used = (uint32_t)face < (uint32_t)p.F;
                if (used) {
                    const float w = L.tv[k][tid] * p.opacity[face];
                    q = p.scale ? w * p.scale[(int64_t)b * p.F + face] : w;
                    if (need_e && (dop || w != 0.f)) {
                        float vk[CH];
                        packed_load<CH>(p.values + at, p.C, c0, p.rvec, vk);
                        float e = 0.f;
#pragma unroll
                        for (int c = 0; c < CH; c++)
                            if (c0 + c < p.C) e += vk[c] * g[c];
                        L.ev[k][tid] += e;
                    }
                }
                if (dval) {
                    float d[CH];
#pragma unroll
                    for (int c = 0; c < CH; c++) d[c] = used ? q * g[c] : 0.f;  // (a literal 0: the upstream may be no number)
                    packed_store<CH>(dval + at, p.C, c0, p.rvec, d);
                }
            }
        }
    }
    if (!dop && !dsc) return;  // uniform
    float R = (gT && S.inside) ? gT[(int64_t)b * S.HW + pix] : 0.f;
    for (int k = p.K - 1; k >= 0; k--) {
        const int face = S.inside ? p.face[list + k * S.HW] : -1;
        const int row = S.inside ? p.row[list + k * S.HW] : -1;
        int key = -1;
        float fg[2] = {0.f, 0.f};  // dL/do_k, dL/ds_k
        if ((uint32_t)face < (uint32_t)p.F && (uint32_t)row < (uint32_t)p.N) {
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

// the arguments both interpolate calls share -> PackedInterpParams
int packed_interp_params(const char* name, int B, int K, int H, int W, int P, int F, int C, int N, const int32_t* face, const float* bary,
                         const int32_t* row, const int32_t* n_used, const int32_t* faces, const float* vert_attrs, PackedInterpParams& p) {
    const PackedRows r = {N, row, n_used};
    if (deferred_interp_params(name, PACKED_MAX_C, B, K, H, W, P, F, C, face, bary, faces, vert_attrs, &r, TAIL_GROUPS, (int64_t)B * K * H * W, p)) return 1;
    p.N = N; p.row = row; p.n_used = n_used;
    return 0;
}

// the arguments both composite_values calls share -> PackedValuesParams (n_used: the backward call's alone, which sets it)
int packed_values_params(const char* name, int B, int K, int H, int W, int F, int C, int N, const int32_t* face, const int32_t* row,
                         const float* faces_opacity, const float* values, const float* face_scale, PackedValuesParams& p) {
    const PackedRows r = {N, row, nullptr};
    if (deferred_values_params(name, PACKED_MAX_C, B, K, H, W, F, C, face, faces_opacity, values, face_scale, &r, TAIL_GROUPS, (int64_t)B * K * H * W, p)) return 1;
    p.rvec = shade_vec(C, values);
    p.N = N; p.row = row; p.n_used = nullptr;
    return 0;
}

template <int KMAX>
void launch_packed_values_backward(const PackedValuesParams& p, hipStream_t st, const float* gi, const float* gt, float* dop, float* dval, float* dsc) {
    const int main_groups = p.B * ValuesBackwardPix::nx(p) * ValuesBackwardPix::ny(p);
    const dim3 groups((unsigned)(main_groups + (dval ? TAIL_GROUPS : 0))), block(256);
    if (p.C <= 4) k_composite_values_packed_backward<KMAX, 4><<<groups, block, 0, st>>>(p, main_groups, gi, gt, dop, dval, dsc);
    else k_composite_values_packed_backward<KMAX, 8><<<groups, block, 0, st>>>(p, main_groups, gi, gt, dop, dval, dsc);
}

}  // namespace
}  // namespace dmr

extern "C" {

int dmr_pack_slots(int B, int K, int H, int W, int F, int capacity, const int32_t* face, int32_t* row, int32_t* n_used, void* stream) {
    using namespace dmr;
    const char* name = "dmr_pack_slots";
    const std::string n = std::string(name) + ": ";
    if (shade_check_sizes(n, B, K, H, W, 0, F, 1, PACKED_MAX_C)) return 1;
    if (capacity < 0) return api_fail((n + "bad rows").c_str());
    if (!face) return api_fail((n + "null fragment lists").c_str());
    const int64_t slots = (int64_t)B * K * H * W;
    if (slots >= (int64_t)1 << 31) return api_fail((n + "problem too large").c_str());
    if (!row || !n_used) return api_fail((n + "null output").c_str());
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int groups = (int)((slots + PACK_SLOTS - 1) / PACK_SLOTS);
    k_pack_count<<<dim3((unsigned)groups), dim3(256), 0, st>>>(face, slots, F, row);
    k_pack_scan<<<dim3(1), dim3(PACK_SCAN), 0, st>>>(row, groups, n_used);
    k_pack_write<<<dim3((unsigned)groups), dim3(256), 0, st>>>(face, slots, F, capacity, row);
    return launched(name);
}

int dmr_interpolate_packed(int B, int K, int H, int W, int P, int F, int C, int N, const int32_t* face, const float* bary,
                           const int32_t* row, const int32_t* n_used, const int32_t* faces, const float* vert_attrs, float* out,
                           void* stream) {
    using namespace dmr;
    const char* name = "dmr_interpolate_packed";
    PackedInterpParams p;
    if (packed_interp_params(name, B, K, H, W, P, F, C, N, face, bary, row, n_used, faces, vert_attrs, p)) return 1;
    if (N == 0) return 0;
    if (!out) return api_fail("dmr_interpolate_packed: null output");
    p.rvec = shade_vec(C, out);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int main_groups = B * p.sx * p.sy;
    const dim3 rows((unsigned)(main_groups + TAIL_GROUPS)), block(256);
    bool via_lds = C > PLAIN_MAX_C && C <= STAGE_MAX_C;
#ifdef DMR_ABLATION
    if ((ablate_bits() & 32768) && C <= STAGE_MAX_C) {  // the other store shape, for profiles/packed/store_shapes.txt
        via_lds = !via_lds;
        if (C <= 4) { k_interpolate_packed<4, true><<<rows, block, 0, st>>>(p, main_groups, out); return launched(name); }
    }
#endif
    if (C <= 4) k_interpolate_packed<4, false><<<rows, block, 0, st>>>(p, main_groups, out);
    else if (via_lds) k_interpolate_packed<8, true><<<rows, block, 0, st>>>(p, main_groups, out);
    else k_interpolate_packed<8, false><<<rows, block, 0, st>>>(p, main_groups, out);
    return launched(name);
}

int dmr_interpolate_packed_backward(int B, int K, int H, int W, int P, int F, int C, int N, const int32_t* face, const float* bary,
                                    const int32_t* row, const int32_t* n_used, const int32_t* faces, const float* vert_attrs,
                                    const float* grad_out, float* dL_dvert_attrs, float* dL_dbary, void* stream) {
    using namespace dmr;
    const char* name = "dmr_interpolate_packed_backward";
    PackedInterpParams p;
    if (packed_interp_params(name, B, K, H, W, P, F, C, N, face, bary, row, n_used, faces, vert_attrs, p)) return 1;
    if (N > 0 && !grad_out) return api_fail("dmr_interpolate_packed_backward: null grad_out");
    if (!dL_dvert_attrs && !dL_dbary) return 0;
    p.rvec = shade_vec(C, grad_out);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    zero_on(st, dL_dvert_attrs, (int64_t)P * C, nullptr, 0, nullptr, 0);
    if (launched(name)) return 1;
    const dim3 groups((unsigned)(B * InterpBackwardPix::nx(p) * InterpBackwardPix::ny(p))), block(256);
    if (C <= 4) k_interpolate_packed_backward<4><<<groups, block, 0, st>>>(p, grad_out, dL_dvert_attrs, dL_dbary);
    else k_interpolate_packed_backward<8><<<groups, block, 0, st>>>(p, grad_out, dL_dvert_attrs, dL_dbary);
    return launched(name);
}

int dmr_composite_values_packed(int B, int K, int H, int W, int F, int C, int N, const int32_t* face, const int32_t* row,
                                const float* faces_opacity, const float* values, const float* face_scale, float* image, float* T,
                                void* stream) {
    using namespace dmr;
    const char* name = "dmr_composite_values_packed";
    PackedValuesParams p;
    if (packed_values_params(name, B, K, H, W, F, C, N, face, row, faces_opacity, values, face_scale, p)) return 1;
    if (!image || !T) return api_fail("dmr_composite_values_packed: null output");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 rows((unsigned)(B * p.sx * p.sy)), block(256);
    if (C <= 4) k_composite_values_packed<4><<<rows, block, 0, st>>>(p, image, T);
    else k_composite_values_packed<16><<<rows, block, 0, st>>>(p, image, T);
    return launched(name);
}

int dmr_composite_values_packed_backward(int B, int K, int H, int W, int F, int C, int N, const int32_t* face, const int32_t* row,
                                         const int32_t* n_used, const float* faces_opacity, const float* values,
                                         const float* face_scale, const float* grad_image, const float* grad_T,
                                         float* dL_dfaces_opacity, float* dL_dvalues, float* dL_dface_scale, void* stream) {
    using namespace dmr;
    const char* name = "dmr_composite_values_packed_backward";
    PackedValuesParams p;
    if (packed_values_params(name, B, K, H, W, F, C, N, face, row, faces_opacity, values, face_scale, p)) return 1;
    if (!n_used) return api_fail("dmr_composite_values_packed_backward: null n_used");
    if (dL_dface_scale && !face_scale) return api_fail("dmr_composite_values_packed_backward: dL_dface_scale without face_scale");
    if (N == 0) dL_dvalues = nullptr;  // (no row to write)
    if (!dL_dfaces_opacity && !dL_dvalues && !dL_dface_scale) return 0;
    p.n_used = n_used;
    p.rvec = p.rvec && (!dL_dvalues || shade_vec(C, dL_dvalues));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    float *dop, *dval, *dsc;
    const int go = values_backward_prologue(name, st, B, F, (int64_t)N * C, grad_image, grad_T, dL_dfaces_opacity, dL_dvalues, dL_dface_scale,
                                            dop, dval, dsc);
    if (go != SHADE_LAUNCH) return go;
    with_kmax(K, [&](auto kmax) {
        launch_packed_values_backward<decltype(kmax)::value>(p, st, grad_image, grad_T, dop, dval, dsc);
    });
    return launched(name);
}

}  // extern "C"
