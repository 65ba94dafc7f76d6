// dmr_hashgrid.hip -- a multiresolution hash-grid encoding of packed rows of 3-D points (include/dmesh_renderer_amd_hashgrid.h):
// the learned field in front of dmr_mlp.hip's MLP, one forward and one backward kernel.  The model is fragments.hashgrid_rows:
//     u_c = clamp(u, 0, 1) (NaN: 0)   p = u_c R_l   i = min(floor(p), R_l - 1)   t = p - i
//     y[r, l F + f] = sum_c w_c table[offsets[l] + row_l(i + c), f]      (8 corners c, trilinear w_c)
// A LANE OWNS A ROW and walks the levels.  The forward gathers 8 table rows per level and stores y through a per-wave LDS
// transpose, 16 channels at a time, so that consecutive lanes store consecutive addresses.  The backward takes the same walk:
// dL/dx recomputes the eight table rows (a plain store per row), dL/dtable is a scatter-add that sums on chip what shares a
// destination before anything leaves -- the lanes of a wave that hold the same table row merge (shade_merge), the survivors
// add into a per-workgroup LDS table of f64 cells keyed by the table row, and the table leaves with one float atomic per cell;
// what the table refuses, and the levels whose lanes do not merge, go out as direct atomics.
//
// Rows r >= min(max(n_rows[0], 0), N) are not read.  Every table row index is clamped (dense level) or masked (hashed level) into
// its level's slice as the last step before the access.  Offsets into y, grad_out and table are int64_t.
#include "dmr_rows_common.hpp"
#include "../../include/dmesh_renderer_amd_hashgrid.h"

namespace dmr {
namespace {

#pragma clang fp contract(fast)

constexpr int HG_MAX_L = DMR_HASHGRID_MAX_LEVELS, HG_THREADS = 256, HG_MAX_GROUPS = DMR_HASHGRID_MAX_GROUPS;
constexpr int HG_CHUNK = 16, HG_PITCH = HG_CHUNK + 1;  // the forward's LDS transpose: channels per flush, a lane's row of them
constexpr uint32_t HG_PRIME_Y = 2654435761u, HG_PRIME_Z = 805459861u;
// the backward's LDS table: slots of a key and F f64 cells (48, 40, 36, 34 KiB for F = 1, 2, 4, 8)
constexpr int hg_slots(int f) { return 4096 / f; }
constexpr int HG_PROBES = 8;
// DMR_ABLATE bits of the ablation build (scripts/time_hashgrid.py); DMR_DBG folds to false in the product
constexpr int HG_FWD_PER_CHUNK = 1 << 20, HG_FWD_LANE_STORE = 1 << 21, HG_BWD_NO_TABLE = 1 << 22, HG_BWD_STATS = 1 << 23, HG_BWD_LANE_ATOMICS = 1 << 24;
#ifdef DMR_ABLATION
__device__ unsigned long long g_hg_stats[HG_MAX_L][2];  // per level: contributions to dL/dtable, and those that left as direct atomics
#endif

struct HgParams {
    int N, L, C;           // C = L * F
    uint32_t dense;        // bit l: level l is dense
    int res[HG_MAX_L];     // R_l
    uint32_t off[HG_MAX_L + 1];  // first row of level l (the total is below 2^29)
    const float* __restrict__ x;       // [N,3]
    const float* __restrict__ table;   // [off[L],F]
    const int32_t* __restrict__ n_rows;  // [1] or null
#ifdef DMR_ABLATION
    int dbg;
#endif
};

// a coordinate at a level of resolution R: the cell i in 0 .. R - 1 and t = p - i in [0, 1]
struct HgAxis { int i; float t; };
__device__ __forceinline__ float hg_clamp01(float u) { return u > 0.f ? (u < 1.f ? u : 1.f) : 0.f; }  // NaN -> 0
__device__ __forceinline__ HgAxis hg_axis(float uc, int R) {
    const float pf = __fmul_rn(uc, (float)R);  // (never contracted into t's subtraction: floor and t see the one rounded product, as the model's do)
    int i = (int)floorf(pf);
    i = i < R - 1 ? i : R - 1;
    i = i > 0 ? i : 0;
    return {i, pf - (float)i};
}
// a lane's cell at one level: the base vertex, the three t, and what the level's rows are numbered by
struct HgCell {
    int ix, iy, iz;
    float tx, ty, tz;
    uint32_t first, last, stride;  // the level's first row, its rows - 1, R + 1; stride == 0: hashed, and `last` is T - 1
};
__device__ __forceinline__ HgCell hg_cell(const HgParams& p, int l, float ux, float uy, float uz) {
    const int R = p.res[l];
    const HgAxis a = hg_axis(ux, R), b = hg_axis(uy, R), c = hg_axis(uz, R);
    const bool dense = (p.dense >> l) & 1u;
    return {a.i, b.i, c.i, a.t, b.t, c.t, p.off[l], p.off[l + 1] - p.off[l] - 1u, dense ? (uint32_t)(R + 1) : 0u};
}
// the row of `table` that holds corner c (bit 0: x + 1, bit 1: y + 1, bit 2: z + 1) of the cell: always inside the level's slice
__device__ __forceinline__ uint32_t hg_row(const HgCell& k, int c) {
    const uint32_t ix = (uint32_t)(k.ix + (c & 1)), iy = (uint32_t)(k.iy + ((c >> 1) & 1)), iz = (uint32_t)(k.iz + ((c >> 2) & 1));
    uint32_t r;
    if (k.stride) { r = ix + k.stride * (iy + k.stride * iz); r = r < k.last ? r : k.last; }
    else r = (ix ^ (iy * HG_PRIME_Y) ^ (iz * HG_PRIME_Z)) & k.last;
    return k.first + r;
}
// the trilinear weight of corner c: (wx wy) wz
__device__ __forceinline__ float hg_weight(const HgCell& k, int c) {
    const float wx = (c & 1) ? k.tx : 1.f - k.tx, wy = (c & 2) ? k.ty : 1.f - k.ty, wz = (c & 4) ? k.tz : 1.f - k.tz;
    return wx * wy * wz;
}

// ---------------------------------------------------------------------------
// forward.  A workgroup strides over tiles of 256 rows; a wave owns 64 consecutive rows and its own staging area, so there is
// no workgroup barrier.  VIA_LDS: 16 channels (16 / F levels) at a time go through the wave's [64][17] staging area and leave as
// 64-byte pieces of 4 rows per store instruction; else (the ablation build's other store shape) every lane stores its own row.
// gridDim.y > 1 (the ablation build's other launch shape) deals the chunks of levels to workgroups of their own.
// ---------------------------------------------------------------------------
template <int F, bool VIA_LDS>
__global__ void __launch_bounds__(HG_THREADS)
k_hashgrid_rows(HgParams p, int tiles, float* __restrict__ y) {
    constexpr int LPC = HG_CHUNK / F;  // levels per chunk
    __shared__ float stage[HG_THREADS / 64][64 * HG_PITCH];
    const int tid = threadIdx.x, lane = tid & 63;
    float* st = stage[tid >> 6];
    const int n = rows_used(p);
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t row = (int64_t)tile * HG_THREADS + tid, row0 = row - lane;
        if (row0 >= p.N) continue;  // (wave-uniform)
        const bool active = row < n;
        float ux = 0.f, uy = 0.f, uz = 0.f;
        if (active) { ux = hg_clamp01(p.x[row * 3]); uy = hg_clamp01(p.x[row * 3 + 1]); uz = hg_clamp01(p.x[row * 3 + 2]); }
        for (int l0 = (int)blockIdx.y * LPC; l0 < p.L; l0 += (int)gridDim.y * LPC) {
#pragma unroll
            for (int k = 0; k < LPC; k++) {
                const int l = l0 + k;
                if (l >= p.L) break;  // (uniform)
                float acc[F];
#pragma unroll
                for (int f = 0; f < F; f++) acc[f] = 0.f;
                if (active) {
                    const HgCell cell = hg_cell(p, l, ux, uy, uz);
#pragma unroll
                    for (int c = 0; c < 8; c++) {
                        const float* __restrict__ tr = p.table + (int64_t)hg_row(cell, c) * F;
                        const float w = hg_weight(cell, c);
#pragma unroll
                        for (int f = 0; f < F; f++) acc[f] += w * tr[f];
                    }
                }
                if constexpr (VIA_LDS) {
#pragma unroll
                    for (int f = 0; f < F; f++) st[lane * HG_PITCH + k * F + f] = acc[f];
                } else if (row < p.N) {
#pragma unroll
                    for (int f = 0; f < F; f++) y[row * p.C + l * F + f] = acc[f];
                }
            }
            if constexpr (VIA_LDS) {
                rows_wave_sync();
                const int c0 = l0 * F, cw = p.C - c0 < HG_CHUNK ? p.C - c0 : HG_CHUNK;
#pragma unroll
                for (int i = 0; i < HG_CHUNK; i++) {
                    const int e = i * 64 + lane, r = e / HG_CHUNK, c = e % HG_CHUNK;
                    if (c < cw && row0 + r < p.N) y[(row0 + r) * p.C + c0 + c] = st[r * HG_PITCH + c];
                }
                rows_wave_sync();
            }
        }
    }
}

// ---------------------------------------------------------------------------
// backward.  A workgroup takes a contiguous run of row tiles (neighbouring rows are neighbouring pixels: what they share stays in
// one workgroup's table).  WX: dL/dx, from the eight table rows of every level; no atomics.  WT: dL/dtable, reads no table:
// per level and corner the lanes of equal table row merge inside their 16-lane DPP rows; if that at least halved the wave's
// contributions, or the whole level fits half the table, the survivors go to the LDS table (open addressing, HG_PROBES probes,
// f64 cells), else -- a fine level, whose rows nobody shares -- straight out as float atomics, like what the table refuses.
// The table leaves when a tile has filled more than half of it, and at the end.
// ---------------------------------------------------------------------------
template <int SLOTS>
__device__ __forceinline__ int hg_find(uint32_t* __restrict__ key, uint32_t rid, int* __restrict__ filled) {
    uint32_t s = __umulhi(rid * 2654435761u, (uint32_t)SLOTS);
    for (int i = 0; i < HG_PROBES; i++) {
        const uint32_t prev = atomicCAS(&key[s], STAB_EMPTY, rid);
        if (prev == STAB_EMPTY) { atomicAdd(filled, 1); return (int)s; }
        if (prev == rid) return (int)s;
        s = s + 1u == (uint32_t)SLOTS ? 0u : s + 1u;
    }
    return -1;
}

// dL/dtable[row[lane]] += v[lane] for the lanes with row >= 0, as float atomics.  F = 2 or 4: the F lanes of a group take the
// group's rows one after the other, lane f of the group adding feature f -- an atomic instruction then touches 16 or 32 segments
// of 16 or 8 bytes instead of 64 single floats in 64 rows (`grouped`; the ablation build can run the other form).  Called by all
// 64 lanes.
template <int F>
__device__ __forceinline__ void hg_add_rows(int lane, int row, const float (&v)[F], float* __restrict__ dtable, bool grouped) {
    if ((F == 2 || F == 4) && grouped) {
        const int sub = lane & (F - 1), first = lane & ~(F - 1);
#pragma unroll
        for (int j = 0; j < F; j++) {
            const int r = __shfl(row, first + j);
            float mine = 0.f;
#pragma unroll
            for (int f = 0; f < F; f++) {
                const float other = __shfl(v[f], first + j);
                mine = sub == f ? other : mine;
            }
            if (r >= 0) unsafeAtomicAdd(&dtable[(int64_t)r * F + sub], mine);
        }
    } else if (row >= 0) {
#pragma unroll
        for (int f = 0; f < F; f++) unsafeAtomicAdd(&dtable[(int64_t)row * F + f], v[f]);
    }
}

template <int F, bool WX, bool WT>
__global__ void __launch_bounds__(HG_THREADS)
k_hashgrid_rows_backward(HgParams p, int tiles, const float* __restrict__ gout, float* __restrict__ dx, float* __restrict__ dtable) {
    constexpr int SLOTS = WT ? hg_slots(F) : 1;
    __shared__ uint32_t key[SLOTS];
    __shared__ double val[SLOTS][F];
    __shared__ int filled;
    const int tid = threadIdx.x, lane = tid & 63;
    if constexpr (WT) {
        for (int s = tid; s < SLOTS; s += HG_THREADS) {
            key[s] = STAB_EMPTY;
#pragma unroll
            for (int f = 0; f < F; f++) val[s][f] = 0.0;
        }
        if (tid == 0) filled = 0;
        __syncthreads();
    }
    const auto flush = [&]() {  // (between two barriers) every cell leaves with one float atomic, the table is empty again
        for (int s = tid; s < SLOTS; s += HG_THREADS) {
            const uint32_t k = key[s];
            if (k == STAB_EMPTY) continue;
#pragma unroll
            for (int f = 0; f < F; f++) { unsafeAtomicAdd(&dtable[(int64_t)k * F + f], (float)val[s][f]); val[s][f] = 0.0; }
            key[s] = STAB_EMPTY;
        }
        if (tid == 0) filled = 0;
    };
    const int n = rows_used(p);
    const RowsTileRun run = rows_tile_run(tiles);
    for (int tile = run.t0; tile < run.t1; tile++) {
        const int64_t row = (int64_t)tile * HG_THREADS + tid;
        const bool active = row < n;
        const unsigned long long live = __ballot(active);
        float d[3] = {0.f, 0.f, 0.f};
        if (live != 0ull) {  // (wave-uniform: the merge below runs with all 64 lanes)
            float ux = 0.f, uy = 0.f, uz = 0.f;
            bool px = false, py = false, pz = false;  // the clamp passes the gradient: 0 <= u <= 1 (false for NaN)
            if (active) {
                const float x0 = p.x[row * 3], x1 = p.x[row * 3 + 1], x2 = p.x[row * 3 + 2];
                px = x0 >= 0.f && x0 <= 1.f; py = x1 >= 0.f && x1 <= 1.f; pz = x2 >= 0.f && x2 <= 1.f;
                ux = hg_clamp01(x0); uy = hg_clamp01(x1); uz = hg_clamp01(x2);
            }
            const int total = __popcll(live);
            for (int l = 0; l < p.L; l++) {
                float g[F];
#pragma unroll
                for (int f = 0; f < F; f++) g[f] = active ? gout[row * p.C + l * F + f] : 0.f;
                const HgCell cell = hg_cell(p, l, ux, uy, uz);
                [[maybe_unused]] const bool small = p.off[l + 1] - p.off[l] <= (uint32_t)(SLOTS / 2);
                float dl[3] = {0.f, 0.f, 0.f};
#pragma unroll
                for (int c = 0; c < 8; c++) {
                    const uint32_t r = hg_row(cell, c);
                    if constexpr (WX) {
                        if (active) {
                            const float* __restrict__ tr = p.table + (int64_t)r * F;
                            float s = 0.f;
#pragma unroll
                            for (int f = 0; f < F; f++) s += tr[f] * g[f];
                            const float wx = (c & 1) ? cell.tx : 1.f - cell.tx, wy = (c & 2) ? cell.ty : 1.f - cell.ty, wz = (c & 4) ? cell.tz : 1.f - cell.tz;
                            dl[0] += ((c & 1) ? s : -s) * (wy * wz);
                            dl[1] += ((c & 2) ? s : -s) * (wx * wz);
                            dl[2] += ((c & 4) ? s : -s) * (wx * wy);
                        }
                    }
                    if constexpr (WT) {
                        int k = active ? (int)r : -1;
                        const float w = hg_weight(cell, c);
                        float v[F];
#pragma unroll
                        for (int f = 0; f < F; f++) v[f] = w * g[f];
                        shade_merge(lane, k, v);
                        const int left = __popcll(__ballot(k >= 0));
                        bool to_table = small || 2 * left <= total;  // (wave-uniform)
                        if (DMR_DBG(p, HG_BWD_NO_TABLE)) to_table = false;
                        int slot = -1;
                        if (k >= 0 && to_table) slot = hg_find<SLOTS>(key, (uint32_t)k, &filled);
                        if (slot >= 0) {
#pragma unroll
                            for (int f = 0; f < F; f++) atomicAdd(&val[slot][f], (double)v[f]);
                        }
                        const int out = (k >= 0 && slot < 0) ? k : -1;  // the table did not take it: straight to dL/dtable
                        const unsigned long long direct = __ballot(out >= 0);
                        if (direct != 0ull) hg_add_rows<F>(lane, out, v, dtable, !DMR_DBG(p, HG_BWD_LANE_ATOMICS));  // (wave-uniform: all 64 lanes take part)
#ifdef DMR_ABLATION
                        if (DMR_DBG(p, HG_BWD_STATS) && lane == 0) {
                            atomicAdd(&g_hg_stats[l][0], (unsigned long long)total);
                            atomicAdd(&g_hg_stats[l][1], (unsigned long long)__popcll(direct));
                        }
#endif
                    }
                }
                if constexpr (WX) {
                    const float R = (float)p.res[l];
                    d[0] += R * dl[0]; d[1] += R * dl[1]; d[2] += R * dl[2];
                }
            }
            if constexpr (WX) { d[0] = px ? d[0] : 0.f; d[1] = py ? d[1] : 0.f; d[2] = pz ? d[2] : 0.f; }
        }
        if constexpr (WX) {
            if (row < p.N) { dx[row * 3] = d[0]; dx[row * 3 + 1] = d[1]; dx[row * 3 + 2] = d[2]; }
        }
        if constexpr (WT) {
            __syncthreads();
            const bool full = filled > SLOTS / 2;  // (uniform: read between two barriers, before flush() resets it)
            __syncthreads();
            if (full) flush();
            __syncthreads();
        }
    }
    if constexpr (WT) flush();
}

#pragma clang fp contract(off)

// THE layout rule (the header states it): the rows of level l, dense when (R + 1)^3 <= T
int64_t hg_level_rows(int R, int log2_T, bool* dense) {
    const int64_t T = (int64_t)1 << log2_T, v = (int64_t)R + 1, cube = v * v * v;
    *dense = cube <= T;
    return *dense ? cube : T;
}
int hg_check_levels(const std::string& n, int L) {
    if (L < 1 || L > HG_MAX_L) return api_fail((n + "L must be in 1.." + std::to_string(HG_MAX_L) + ", got " + std::to_string(L)).c_str());
    return 0;
}
int hg_check_table(const std::string& n, int L, int log2_T, const int32_t* resolutions) {
    if (log2_T < 4 || log2_T > 24) return api_fail((n + "log2_T must be in 4..24, got " + std::to_string(log2_T)).c_str());
    if (!resolutions) return api_fail((n + "null resolutions").c_str());
    for (int l = 0; l < L; l++)
        if (resolutions[l] < 1 || resolutions[l] > 65536)
            return api_fail((n + "resolutions[" + std::to_string(l) + "] must be in 1..65536, got " + std::to_string(resolutions[l])).c_str());
    return 0;
}

// what both calls check first, in the header's order -> HgParams
int hg_params(const char* name, int N, int L, int F, int log2_T, const int32_t* resolutions, const float* x, const float* table,
              const int32_t* n_rows, HgParams& p) {
    const std::string n = std::string(name) + ": ";
    if (N < 0) return api_fail((n + "bad rows").c_str());
    if (hg_check_levels(n, L)) return 1;
    if (F != 1 && F != 2 && F != 4 && F != 8) return api_fail((n + "F must be 1, 2, 4 or 8, got " + std::to_string(F)).c_str());
    if (L * F > DMR_HASHGRID_MAX_CHANNELS) return api_fail((n + "L * F must be at most " + std::to_string(DMR_HASHGRID_MAX_CHANNELS) + ", got " + std::to_string(L * F)).c_str());
    if (hg_check_table(n, L, log2_T, resolutions)) return 1;
    if (N > 0 && !x) return api_fail((n + "null x").c_str());
    if (!table) return api_fail((n + "null table").c_str());
    p.N = N; p.L = L; p.C = L * F; p.dense = 0u;
    int64_t off = 0;
    for (int l = 0; l < HG_MAX_L; l++) {
        p.res[l] = l < L ? resolutions[l] : 1;
        p.off[l] = (uint32_t)off;
        if (l < L) {
            bool dense;
            off += hg_level_rows(resolutions[l], log2_T, &dense);
            if (dense) p.dense |= 1u << l;
        }
    }
    p.off[HG_MAX_L] = (uint32_t)off;
    p.x = x; p.table = table; p.n_rows = n_rows;
#ifdef DMR_ABLATION
    p.dbg = ablate_bits();
#endif
    return 0;
}

}  // namespace
}  // namespace dmr

extern "C" {

int dmr_hashgrid_layout(int L, int log2_T, const int32_t* resolutions, int64_t* offsets_out) {
    using namespace dmr;
    const std::string n = "dmr_hashgrid_layout: ";
    if (hg_check_levels(n, L) || hg_check_table(n, L, log2_T, resolutions)) return 1;
    if (!offsets_out) return api_fail((n + "null output").c_str());
    int64_t off = 0;
    for (int l = 0; l < L; l++) {
        bool dense;
        offsets_out[l] = off;
        off += hg_level_rows(resolutions[l], log2_T, &dense);
    }
    offsets_out[L] = off;
    return 0;
}

int dmr_hashgrid_rows(int N, int L, int F, int log2_T, const int32_t* resolutions, const float* x, const float* table,
                      const int32_t* n_rows, float* y, void* stream) {
    using namespace dmr;
    const char* name = "dmr_hashgrid_rows";
    HgParams p;
    if (hg_params(name, N, L, F, log2_T, resolutions, x, table, n_rows, p)) return 1;
    if (N == 0) return 0;
    if (!y) return api_fail("dmr_hashgrid_rows: null output");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const RowsGrid g = rows_grid(N, HG_THREADS, HG_MAX_GROUPS);
    dim3 groups((unsigned)g.groups), block(HG_THREADS);
    with_one_of<1, 2, 4, 8>(F, [&](auto f) {  // (the 4 instantiations of the forward)
        constexpr int FF = decltype(f)::value;
#ifdef DMR_ABLATION
        if (p.dbg & HG_FWD_PER_CHUNK) groups.y = (unsigned)((L * FF + HG_CHUNK - 1) / HG_CHUNK);  // a (row block, chunk of levels) grid
        if (p.dbg & HG_FWD_LANE_STORE) { k_hashgrid_rows<FF, false><<<groups, block, 0, st>>>(p, g.tiles, y); return; }
#endif
        k_hashgrid_rows<FF, true><<<groups, block, 0, st>>>(p, g.tiles, y);
    });
    return launched(name);
}

int dmr_hashgrid_rows_backward(int N, int L, int F, int log2_T, const int32_t* resolutions, const float* x, const float* table,
                               const int32_t* n_rows, const float* grad_out, float* dL_dx, float* dL_dtable, void* stream) {
    using namespace dmr;
    const char* name = "dmr_hashgrid_rows_backward";
    HgParams p;
    if (hg_params(name, N, L, F, log2_T, resolutions, x, table, n_rows, p)) return 1;
    const int go = rows_backward_prologue(name, N, grad_out, nullptr, dL_dx, dL_dtable != nullptr);
    if (go != SHADE_LAUNCH) return go;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (dL_dtable) {  // zeroed before the backward adds into it
        rows_fill_on(st, dL_dtable, (int64_t)p.off[HG_MAX_L] * F, 0u);
        if (launched(name)) return 1;
    }
    if (N == 0) return 0;
    const RowsGrid g = rows_grid(N, HG_THREADS, HG_MAX_GROUPS);
    const dim3 groups((unsigned)g.groups), block(HG_THREADS);
    with_one_of<1, 2, 4, 8>(F, [&](auto f) {  // (... the 12 of the backward)
        with_wanted(dL_dx != nullptr, dL_dtable != nullptr, [&](auto wx, auto wt) {  // (an output that is not wanted is null)
            k_hashgrid_rows_backward<decltype(f)::value, decltype(wx)::value, decltype(wt)::value><<<groups, block, 0, st>>>(p, g.tiles, grad_out, dL_dx, dL_dtable);
        });
    });
    return launched(name);
}

#ifdef DMR_ABLATION
// (ablation build only) per level: contributions to dL/dtable and those that left as direct atomics, since the last reset
int dmr_hashgrid_stats(unsigned long long* out, int reset) {
    using namespace dmr;
    static const unsigned long long zeros[HG_MAX_L][2] = {};
    if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(g_hg_stats), sizeof(zeros)) != hipSuccess) return api_fail("dmr_hashgrid_stats: copy failed");
    if (reset && hipMemcpyToSymbol(HIP_SYMBOL(g_hg_stats), zeros, sizeof(zeros)) != hipSuccess) return api_fail("dmr_hashgrid_stats: reset failed");
    return 0;
}
#endif

}  // extern "C"
