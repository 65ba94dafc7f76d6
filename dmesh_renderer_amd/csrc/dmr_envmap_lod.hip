// dmr_envmap_lod.hip -- a mip pyramid of a learnable lat-long environment map and direction rows looked up in it at a per-row
// level of detail (include/dmesh_renderer_amd_envmap_lod.h): the specular term of a rough surface.  The builder (one launch per
// level, and one gather launch for its backward) and the lookup (one forward and one backward kernel).  The models are
// fragments.envmap_pyramid and fragments.envmap_lod_rows:
//     level l+1 at (i, j) = ((a + b) + (c + d)) * 0.25 of level l's 2 x 2 block; level 0 is the base map
//     y[r] = (1-f) B_l0 + f B_l1,  B_l = dmr_envmap.hip's bilinear mix at level l,  (l0, l1, f) from lod[r] (env_lod_levels)
// The lookup follows dmr_envmap.hip: A LANE OWNS A ROW.  The two atan2f, the square root and the normalisation run once per row
// (env_angles); the eight texel addresses and weights are then formed from (s, t) per level (env_place), the channels go in
// chunks of four, as float4 texel reads when C % 4 == 0 and the pyramid is 16-byte aligned, and y leaves row by row or through
// the per-wave LDS transpose -- dmr_envmap.hip's choice per chunk count, kept unmeasured (profiles/envmap_lod/store_shapes.txt).
// The backward is a template of what is wanted, <WD, WL, WP>: dL/dd and dL/dlod are plain stores per row; dL/dpyramid is
// dmr_envmap.hip's scatter-add on the texture unit's machinery: the lanes of a wave that hold the same (texel, chunk) merge
// (shade_merge), the survivors add into a per-workgroup LDS table of f64 cells (stab_find_n), the table leaves as float atomics
// when more than half full and at the end, and what the table refuses goes out as direct atomics.
//
// Memory safety does not depend on the input bits: wrap_pair is the last step before a level's four indices and the clamp into
// [0, L-1] the last before the two levels (dmr_envmap_lod_coords.hpp, plain C++ the CPU tests run on the host), and every load,
// LDS key and atomic below takes its level and texel from there.  Rows r >= min(max(n_rows[0], 0), N) are not read.  Offsets
// into y, grad_out, lod and the pyramid are int64_t.
#include "dmr_rows_common.hpp"
#include "dmr_envmap_lod_coords.hpp"
#include "../../include/dmesh_renderer_amd_envmap_lod.h"

namespace dmr {
namespace {

constexpr int LOD_THREADS = 256, LOD_MAX_GROUPS = DMR_ENVMAP_LOD_MAX_GROUPS, LOD_MAX_C = DMR_ENVMAP_LOD_MAX_CHANNELS, LOD_MAX_L = DMR_ENVMAP_LOD_MAX_LEVELS;
static_assert(LOD_MAX_L == ENV_LOD_MAX_LEVELS, "the public header and dmr_envmap_lod_coords.hpp state the same limit");
// the shape of y's stores per chunk count (1, 2, 4: C <= 4, <= 8, <= 16): through the LDS transpose, or every lane its row.
// dmr_envmap.hip's choice, kept unmeasured
constexpr bool lod_via_lds(int nch) { return nch >= 2; }
constexpr int lod_pitch(int nch) { return (4 * nch) | 1; }  // (an odd row pitch: a wave's lanes on distinct banks)
constexpr size_t lod_stage_bytes(int nch, bool via_lds) { return via_lds ? (size_t)(LOD_THREADS / 64) * 64 * lod_pitch(nch) * sizeof(float) : 0; }
extern __shared__ __attribute__((aligned(16))) unsigned char lod_lds[];
// The backward's table of texel gradients: keyed by texel x channel chunk, four f64 sums per cell; dmr_envmap.hip's size
constexpr int LOD_TAB = 1024;
// DMR_ABLATE bit of the ablation build (scripts/time_envmap_lod.py): count what leaves as direct atomics
[[maybe_unused]] constexpr int LOD_STATS = 1 << 28;
#ifdef DMR_ABLATION
__device__ unsigned long long g_lod_stats[2];  // contributions to dL/dpyramid (a row's texel x chunk), and those that left as direct atomics
#endif
constexpr int PYR_THREADS = 256, PYR_MAX_GROUPS = 4096;  // the builder's launches: a float (the copy) or a texel per thread, further ones in a loop

// ---------------------------------------------------------------------------
// The builder.  Not contracted (the build's -ffp-contract=off): the sums below are the model's, operation by operation.
// ---------------------------------------------------------------------------
// level 0 <- the base map: n floats
__global__ void __launch_bounds__(PYR_THREADS)
k_envmap_pyramid_base(const float* __restrict__ env, float* __restrict__ pyr, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * PYR_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * PYR_THREADS) pyr[i] = env[i];
}

// dst [Hd,Wd,C] <- the 2 x 2 blocks of src [2 Hd, 2 Wd, C]; a thread per texel of dst (32-bit index arithmetic: a level above
// the base has fewer than 2^29 texels), its channels in a loop
__global__ void __launch_bounds__(PYR_THREADS)
k_envmap_pyramid_level(const float* __restrict__ src, float* __restrict__ dst, int Hd, int Wd, int C) {
    const uint32_t n = (uint32_t)Hd * (uint32_t)Wd;
    const int64_t rowf = (int64_t)2 * Wd * C;
    for (uint32_t t = blockIdx.x * PYR_THREADS + threadIdx.x; t < n; t += gridDim.x * PYR_THREADS) {
        const uint32_t y = t / (uint32_t)Wd, x = t - y * (uint32_t)Wd;
        const float* __restrict__ a = src + (int64_t)(2 * y) * rowf + (int64_t)(2 * x) * C;
        float* __restrict__ o = dst + (int64_t)t * C;
        for (int c = 0; c < C; c++) o[c] = ((a[c] + a[C + c]) + (a[rowf + c] + a[rowf + C + c])) * 0.25f;
    }
}

// dL_denvmap [He,We,C] <- grad_pyramid [T,C]: per base texel Horner from the coarsest level down, four channels at a time; a
// gather, no atomics
__global__ void __launch_bounds__(PYR_THREADS)
k_envmap_pyramid_backward(const float* __restrict__ g, float* __restrict__ denv, int He, int We, int C, int L) {
    const uint32_t n = (uint32_t)He * (uint32_t)We;
    for (uint32_t t = blockIdx.x * PYR_THREADS + threadIdx.x; t < n; t += gridDim.x * PYR_THREADS) {
        const uint32_t y = t / (uint32_t)We, x = t - y * (uint32_t)We;
        for (int c0 = 0; c0 < C; c0 += 4) {
            float acc[4] = {0.f, 0.f, 0.f, 0.f};
            for (int l = L - 1; l >= 0; l--) {
                const uint32_t at = env_lod_offset(He, We, l) + (y >> l) * (uint32_t)(We >> l) + (x >> l);
                const float* __restrict__ row = g + (int64_t)at * C + c0;
#pragma unroll
                for (int j = 0; j < 4; j++)
                    if (c0 + j < C) acc[j] = row[j] + 0.25f * acc[j];
            }
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (c0 + j < C) denv[(int64_t)t * C + c0 + j] = acc[j];
        }
    }
}

#pragma clang fp contract(fast)

struct LodParams {
    int N, C, He, We, L;
    int nch;  // ceil(C / 4): channel chunks per texel
    int vec;  // a texel's chunk may be read as float4 (C % 4 == 0, 16-byte aligned base)
    int lod_stride;
    const float* __restrict__ d;         // [N,3]
    const float* __restrict__ lod;       // [N], lod_stride floats apart
    const float* __restrict__ pyr;       // [T,C]
    const int32_t* __restrict__ n_rows;  // [1] or null
#ifdef DMR_ABLATION
    int dbg;
#endif
};

// A row as the kernels see it: whether it is used; per level k of its two (l0, l1) the level's weight w[k] = (1-f, f), its size,
// its four texels (rows of the pyramid: 00 = (iy0, ix0), 01 = (iy0, ix1), 10, 11) and its cell's fractions; what dL/dd needs
// beside them.
struct LodRow {
    bool used, pole, inside;
    float w[2];
    int He[2], We[2];
    uint32_t t[2][4];
    float fx[2], fy[2];
    float ux, uy, uz, inv, rho2;
};
__device__ __forceinline__ LodRow lod_row(const LodParams& p, int64_t row, int n) {
    LodRow r = {};
    if (row >= n) return r;
    const EnvAngles a = env_angles(p.d[row * 3], p.d[row * 3 + 1], p.d[row * 3 + 2]);
    if (a.skipped) return r;
    const EnvLodLevels v = env_lod_levels(p.lod[row * p.lod_stride], p.L);
    r.used = true; r.pole = a.pole; r.inside = v.inside;
    r.w[0] = 1.f - v.f; r.w[1] = v.f;
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const int l = k ? v.l1 : v.l0;
        r.He[k] = p.He >> l; r.We[k] = p.We >> l;
        const EnvPlace c = env_place(a.s, a.t, r.He[k], r.We[k]);
        const uint32_t off = env_lod_offset(p.He, p.We, l);
        const uint32_t r0 = off + (uint32_t)c.iy0 * (uint32_t)r.We[k], r1 = off + (uint32_t)c.iy1 * (uint32_t)r.We[k];
        r.t[k][0] = r0 + (uint32_t)c.ix0; r.t[k][1] = r0 + (uint32_t)c.ix1; r.t[k][2] = r1 + (uint32_t)c.ix0; r.t[k][3] = r1 + (uint32_t)c.ix1;
        r.fx[k] = c.fx; r.fy[k] = c.fy;
    }
    r.ux = a.ux; r.uy = a.uy; r.uz = a.uz; r.inv = a.inv; r.rho2 = a.rho2;
    return r;
}

// channels c0 .. c0 + 3 of the pyramid's row t (0 past C)
__device__ __forceinline__ void lod_texel(const LodParams& p, uint32_t t, int c0, float (&r)[4]) {
    const float* __restrict__ row = p.pyr + (int64_t)t * p.C + c0;
    if (p.vec) {
        const float4 v = *reinterpret_cast<const float4*>(row);
        r[0] = v.x; r[1] = v.y; r[2] = v.z; r[3] = v.w;
    } else {
#pragma unroll
        for (int c = 0; c < 4; c++) r[c] = c0 + c < p.C ? row[c] : 0.f;
    }
}

// ---------------------------------------------------------------------------
// forward: dmr_envmap.hip's, with two levels.  A workgroup strides over tiles of 256 rows; a wave owns 64 consecutive rows and
// its own staging area, so there is no workgroup barrier.  NCH: the chunks of four channels a lane's registers hold (1, 2, 4).
// VIA_LDS: the wave's 64 rows of C floats go through its [64][4 NCH | 1] staging area and leave as 64 C consecutive floats; else
// every lane stores its own row.  A level whose weight is 0 is not read.  A skipped row stores zeros.
// ---------------------------------------------------------------------------
template <int NCH, bool VIA_LDS>
__global__ void __launch_bounds__(LOD_THREADS)
k_envmap_lod_rows(LodParams p, int tiles, float* __restrict__ y) {
    constexpr int PITCH = lod_pitch(NCH);
    const int tid = threadIdx.x, lane = tid & 63, C = p.C;
    [[maybe_unused]] float* st = reinterpret_cast<float*>(lod_lds) + (tid >> 6) * (64 * PITCH);  // (VIA_LDS) the wave's staging area
    const int n = rows_used(p);
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t row = (int64_t)tile * LOD_THREADS + tid, row0 = row - lane;
        if (row0 >= p.N) continue;  // (wave-uniform)
        const LodRow r = lod_row(p, row, n);
        float o[4 * NCH];
#pragma unroll
        for (int c = 0; c < 4 * NCH; c++) o[c] = 0.f;
        if (r.used) {
#pragma unroll
            for (int k = 0; k < 2; k++) {
                if (r.w[k] == 0.f) continue;
                const float ax = 1.f - r.fx[k], ay = 1.f - r.fy[k];
                const float w00 = ay * ax, w01 = ay * r.fx[k], w10 = r.fy[k] * ax, w11 = r.fy[k] * r.fx[k];
#pragma unroll
                for (int i = 0; i < NCH; i++) {
                    if (4 * i >= C) break;  // (uniform)
                    float r0[4], r1[4], r2[4], r3[4];
                    lod_texel(p, r.t[k][0], 4 * i, r0); lod_texel(p, r.t[k][1], 4 * i, r1);
                    lod_texel(p, r.t[k][2], 4 * i, r2); lod_texel(p, r.t[k][3], 4 * i, r3);
#pragma unroll
                    for (int j = 0; j < 4; j++) o[4 * i + j] += r.w[k] * (w00 * r0[j] + w01 * r1[j] + w10 * r2[j] + w11 * r3[j]);
                }
            }
        }
        if constexpr (VIA_LDS) {
#pragma unroll
            for (int c = 0; c < 4 * NCH; c++) st[lane * PITCH + c] = o[c];
            rows_wave_sync();
            const int64_t left = ((int64_t)p.N - row0) * C;  // the floats of y from the wave's first row on
            for (int i = 0; i < C; i++) {
                const int e = i * 64 + lane, er = e / C;
                if (e < left) y[row0 * C + e] = st[er * PITCH + (e - er * C)];
            }
            rows_wave_sync();
        } else if (row < p.N) {
#pragma unroll
            for (int c = 0; c < 4 * NCH; c++)
                if (c < C) y[row * C + c] = o[c];
        }
    }
}

// ---------------------------------------------------------------------------
// backward.  A workgroup takes a contiguous run of row tiles: neighbouring rows share texels, and stay in one workgroup's
// table.  Per row the two levels' texels and fractions once; then per chunk of four channels and per level k
//   WD, WL: e_i = texel_i . g of the four texels (read where the level's weight is not 0, and at both levels where WL and inside)
//       WD: Gx_k += (1-fy)(e01 - e00) + fy (e11 - e10), Gy_k alike; after the chunks Gphi = sum_k w_k (We_k / 2 pi) Gx_k, Gtheta alike,
//           then dmr_envmap.hip's chain, one plain store per row (zeros in a skipped row and at a pole);
//       WL: Bg_k += the bilinear mix of the e_i; dL/dlod = Bg_1 - Bg_0 where inside, else 0: one plain store per row;
//   WP: w_k w_i g of the four texels, merged over the wave's lanes of equal (texel, chunk), into the table; a cell the table
//       refuses goes out with direct atomics.  After every tile the workgroup counts the table's keys and lets it leave when more
//       than half full; it leaves at the end.  Every lane of the workgroup runs every tile (merges, barriers).
// ---------------------------------------------------------------------------
template <bool WD, bool WL, bool WP>
__global__ void __launch_bounds__(LOD_THREADS)
k_envmap_lod_rows_backward(LodParams p, int tiles, const float* __restrict__ gout, float* __restrict__ dd, float* __restrict__ dlod,
                           float* __restrict__ dpyr) {
    __shared__ double tval[WP ? LOD_TAB : 1][4];
    __shared__ uint32_t tkey[WP ? LOD_TAB : 1];
    const int tid = threadIdx.x, lane = tid & 63, C = p.C;
    if constexpr (WP) {
        for (int i = tid; i < LOD_TAB; i += LOD_THREADS) {
            tkey[i] = STAB_EMPTY;
#pragma unroll
            for (int c = 0; c < 4; c++) tval[i][c] = 0.0;
        }
        __syncthreads();
    }
    // (between two barriers) every cell leaves, four lanes per cell -- a texel's chunk is 16 contiguous bytes --, and is empty again
    const auto flush = [&]() {
        for (int i = tid; i < LOD_TAB * 4; i += LOD_THREADS) {
            const uint32_t rid = tkey[i >> 2];
            if (rid == STAB_EMPTY) continue;
            const uint32_t t = rid / (uint32_t)p.nch;
            const int c = (int)(rid - t * (uint32_t)p.nch) * 4 + (i & 3);
            const double x = tval[i >> 2][i & 3];
            tval[i >> 2][i & 3] = 0.0;
            if (c < C && x != 0.0) unsafeAtomicAdd(&dpyr[(int64_t)t * C + c], (float)x);
        }
        __syncthreads();
        for (int i = tid; i < LOD_TAB; i += LOD_THREADS) tkey[i] = STAB_EMPTY;
    };
    const int n = rows_used(p);
    const RowsTileRun run = rows_tile_run(tiles);
    for (int tile = run.t0; tile < run.t1; tile++) {
        const int64_t row = (int64_t)tile * LOD_THREADS + tid;
        const LodRow r = lod_row(p, row, n);
        float out[3] = {0.f, 0.f, 0.f}, slope = 0.f;
        if (__ballot(r.used) != 0ull) {  // (wave-uniform: the merge below runs with all 64 lanes)
            float Gx[2] = {0.f, 0.f}, Gy[2] = {0.f, 0.f}, Bg[2] = {0.f, 0.f};
            for (int c0 = 0, ch = 0; c0 < C; c0 += 4, ch++) {  // (uniform)
                float g[4];
#pragma unroll
                for (int j = 0; j < 4; j++) g[j] = (r.used && c0 + j < C) ? gout[row * C + c0 + j] : 0.f;
#pragma unroll
                for (int k = 0; k < 2; k++) {
                    const float ax = 1.f - r.fx[k], ay = 1.f - r.fy[k];
                    const float w[4] = {ay * ax, ay * r.fx[k], r.fy[k] * ax, r.fy[k] * r.fx[k]};
                    if constexpr (WD || WL) {
                        if (r.used && ((WD && r.w[k] != 0.f) || (WL && r.inside))) {
                            float r0[4], r1[4], r2[4], r3[4];
                            lod_texel(p, r.t[k][0], c0, r0); lod_texel(p, r.t[k][1], c0, r1);
                            lod_texel(p, r.t[k][2], c0, r2); lod_texel(p, r.t[k][3], c0, r3);
                            float e0 = 0.f, e1 = 0.f, e2 = 0.f, e3 = 0.f;
#pragma unroll
                            for (int j = 0; j < 4; j++) { e0 += r0[j] * g[j]; e1 += r1[j] * g[j]; e2 += r2[j] * g[j]; e3 += r3[j] * g[j]; }
                            if constexpr (WD) {
                                if (r.w[k] != 0.f) {  // (a level read for dL/dlod alone stays out of dL/dd: a non-finite texel there reaches only dL/dlod)
                                    Gx[k] += ay * (e1 - e0) + r.fy[k] * (e3 - e2);
                                    Gy[k] += ax * (e2 - e0) + r.fx[k] * (e3 - e1);
                                }
                            }
                            if constexpr (WL) Bg[k] += w[0] * e0 + w[1] * e1 + w[2] * e2 + w[3] * e3;
                        }
                    }
                    if constexpr (WP) {
#pragma unroll
                        for (int i = 0; i < 4; i++) {
                            const float wi = r.w[k] * w[i];
                            const bool adds = r.used && wi != 0.f;
                            int key = adds ? (int)(r.t[k][i] * (uint32_t)p.nch + (uint32_t)ch) : -1;
                            float v[4];
#pragma unroll
                            for (int j = 0; j < 4; j++) v[j] = wi * g[j];
                            shade_merge(lane, key, v);
                            int slot = -1;
                            if (key >= 0) slot = stab_find_n<LOD_TAB>(tkey, (uint32_t)key);
                            if (key >= 0) {
#pragma unroll
                                for (int j = 0; j < 4; j++) {
                                    if (c0 + j >= C) continue;
                                    if (slot >= 0) atomicAdd(&tval[slot][j], (double)v[j]);
                                    else unsafeAtomicAdd(&dpyr[(int64_t)r.t[k][i] * C + c0 + j], v[j]);
                                }
                            }
#ifdef DMR_ABLATION
                            if (DMR_DBG(p, LOD_STATS)) {
                                const unsigned long long all = __ballot(adds), direct = __ballot(key >= 0 && slot < 0);
                                if (lane == 0) { atomicAdd(&g_lod_stats[0], (unsigned long long)__popcll(all)); atomicAdd(&g_lod_stats[1], (unsigned long long)__popcll(direct)); }
                            }
#endif
                        }
                    }
                }
            }
            if constexpr (WD) {
                if (r.used && !r.pole) {
                    const float Gphi = r.w[0] * ((float)r.We[0] * ENV_INV_2PI) * Gx[0] + r.w[1] * ((float)r.We[1] * ENV_INV_2PI) * Gx[1];
                    const float Gtheta = r.w[0] * ((float)r.He[0] * ENV_INV_PI) * Gy[0] + r.w[1] * ((float)r.He[1] * ENV_INV_PI) * Gy[1];
                    const float ir2 = 1.f / r.rho2;
                    const float gx = -Gphi * r.uy * ir2, gy = Gphi * r.ux * ir2, gz = -Gtheta * sqrtf(ir2);
                    const float radial = r.ux * gx + r.uy * gy + r.uz * gz;
                    out[0] = (gx - r.ux * radial) * r.inv; out[1] = (gy - r.uy * radial) * r.inv; out[2] = (gz - r.uz * radial) * r.inv;
                }
            }
            if constexpr (WL) {
                if (r.used && r.inside) slope = Bg[1] - Bg[0];
            }
        }
        if constexpr (WD) {
            if (row < p.N) { dd[row * 3] = out[0]; dd[row * 3 + 1] = out[1]; dd[row * 3 + 2] = out[2]; }
        }
        if constexpr (WL) {
            if (row < p.N) dlod[row] = slope;
        }
        if constexpr (WP) {
            int filled = 0;  // (uniform: every barrier below returns the workgroup's count)
            for (int i = tid; i < LOD_TAB; i += LOD_THREADS) filled += __syncthreads_count(tkey[i] != STAB_EMPTY);
            if (filled > LOD_TAB / 2) { flush(); __syncthreads(); }
        }
    }
    if constexpr (WP) { __syncthreads(); flush(); }
}

#pragma clang fp contract(off)

// the spec's checks, in the header's order -> T, the pyramid's rows
int lod_spec(const std::string& n, int C, int He, int We, int L, int64_t& T) {
    if (C < 1 || C > LOD_MAX_C) return api_fail((n + "C must be in 1.." + std::to_string(LOD_MAX_C) + ", got " + std::to_string(C)).c_str());
    if (L < 1 || L > LOD_MAX_L) return api_fail((n + "L must be in 1.." + std::to_string(LOD_MAX_L) + ", got " + std::to_string(L)).c_str());
    if (He < 1 || We < 1) return api_fail((n + "the map must have at least one texel").c_str());
    const int mask = (1 << (L - 1)) - 1;
    if ((He & mask) || (We & mask)) return api_fail((n + "He and We must be multiples of 2^(L-1)").c_str());
    T = 0;
    for (int l = 0; l < L; l++) T += (int64_t)(He >> l) * (We >> l);
    if (T * ((C + 3) / 4) >= (int64_t)1 << 31) return api_fail((n + "pyramid too large: T * ceil(C / 4) must be below 2^31").c_str());
    return 0;
}

// what both calls of the lookup check first, in the header's order -> LodParams, T
int lod_params(const char* name, int N, int C, int He, int We, int L, int lod_stride, const float* d, const float* lod, const float* pyramid,
               const int32_t* n_rows, LodParams& p, int64_t& T) {
    const std::string n = std::string(name) + ": ";
    if (N < 0) return api_fail((n + "bad rows").c_str());
    if (lod_spec(n, C, He, We, L, T)) return 1;
    if (lod_stride < 1) return api_fail((n + "lod_stride must be at least 1").c_str());
    if (N > 0 && !d) return api_fail((n + "null d").c_str());
    if (N > 0 && !lod) return api_fail((n + "null lod").c_str());
    if (N > 0 && !pyramid) return api_fail((n + "null pyramid").c_str());
    p.N = N; p.C = C; p.He = He; p.We = We; p.L = L;
    p.nch = (C + 3) / 4;
    p.vec = shade_vec(C, pyramid);
    p.lod_stride = lod_stride;
    p.d = d; p.lod = lod; p.pyr = pyramid; p.n_rows = n_rows;
#ifdef DMR_ABLATION
    p.dbg = ablate_bits();
#endif
    return 0;
}

// f(WD, WL, WP) as bool constants for three outputs of which at least one is wanted: the 7 instantiations of the backward
template <class Fn>
void lod_with_wanted(bool d, bool l, bool pyr, Fn&& f) {
    with_one_of<1, 2, 3, 4, 5, 6, 7>((d ? 1 : 0) | (l ? 2 : 0) | (pyr ? 4 : 0), [&](auto m) {
        constexpr int M = decltype(m)::value;
        f(std::bool_constant<(M & 1) != 0>(), std::bool_constant<(M & 2) != 0>(), std::bool_constant<(M & 4) != 0>());
    });
}

inline dim3 pyr_groups(int64_t n) {
    const int64_t blocks = (n + PYR_THREADS - 1) / PYR_THREADS;
    return dim3((unsigned)(blocks < PYR_MAX_GROUPS ? blocks : PYR_MAX_GROUPS));
}

}  // namespace
}  // namespace dmr

extern "C" {

int dmr_envmap_pyramid(int C, int He, int We, int L, const float* envmap, float* pyramid, void* stream) {
    using namespace dmr;
    const char* name = "dmr_envmap_pyramid";
    int64_t T;
    if (lod_spec(std::string(name) + ": ", C, He, We, L, T)) return 1;
    if (!envmap) return api_fail("dmr_envmap_pyramid: null envmap");
    if (!pyramid) return api_fail("dmr_envmap_pyramid: null output");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int64_t n0 = (int64_t)He * We * C;
    k_envmap_pyramid_base<<<pyr_groups(n0), dim3(PYR_THREADS), 0, st>>>(envmap, pyramid, n0);
    if (launched(name)) return 1;
    for (int l = 1; l < L; l++) {  // (level l from level l - 1, stream-ordered)
        const int Hd = He >> l, Wd = We >> l;
        const float* src = pyramid + (int64_t)env_lod_offset(He, We, l - 1) * C;
        k_envmap_pyramid_level<<<pyr_groups((int64_t)Hd * Wd), dim3(PYR_THREADS), 0, st>>>(src, pyramid + (int64_t)env_lod_offset(He, We, l) * C, Hd, Wd, C);
        if (launched(name)) return 1;
    }
    return 0;
}

int dmr_envmap_pyramid_backward(int C, int He, int We, int L, const float* grad_pyramid, float* dL_denvmap, void* stream) {
    using namespace dmr;
    const char* name = "dmr_envmap_pyramid_backward";
    int64_t T;
    if (lod_spec(std::string(name) + ": ", C, He, We, L, T)) return 1;
    if (!grad_pyramid) return api_fail("dmr_envmap_pyramid_backward: null grad_pyramid");
    if (!dL_denvmap) return api_fail("dmr_envmap_pyramid_backward: null output");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    k_envmap_pyramid_backward<<<pyr_groups((int64_t)He * We), dim3(PYR_THREADS), 0, st>>>(grad_pyramid, dL_denvmap, He, We, C, L);
    return launched(name);
}

int dmr_envmap_lod_rows(int N, int C, int He, int We, int L, int lod_stride, const float* d, const float* lod, const float* pyramid,
                        const int32_t* n_rows, float* y, void* stream) {
    using namespace dmr;
    const char* name = "dmr_envmap_lod_rows";
    LodParams p;
    int64_t T;
    if (lod_params(name, N, C, He, We, L, lod_stride, d, lod, pyramid, n_rows, p, T)) return 1;
    if (N == 0) return 0;
    if (!y) return api_fail("dmr_envmap_lod_rows: null output");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const RowsGrid g = rows_grid(N, LOD_THREADS, LOD_MAX_GROUPS);
    const dim3 groups((unsigned)g.groups), block(LOD_THREADS);
    with_one_of<1, 2, 4>(p.nch, [&](auto nch) {  // (the 3 instantiations of the forward: C <= 4, <= 8, <= 16 -- 3 chunks run as 4)
        constexpr int NCH = decltype(nch)::value;
        constexpr bool S = lod_via_lds(NCH);
        k_envmap_lod_rows<NCH, S><<<groups, block, lod_stage_bytes(NCH, S), st>>>(p, g.tiles, y);
    });
    return launched(name);
}

int dmr_envmap_lod_rows_backward(int N, int C, int He, int We, int L, int lod_stride, const float* d, const float* lod,
                                 const float* pyramid, const int32_t* n_rows, const float* grad_out, float* dL_dd, float* dL_dlod,
                                 float* dL_dpyramid, void* stream) {
    using namespace dmr;
    const char* name = "dmr_envmap_lod_rows_backward";
    LodParams p;
    int64_t T;
    if (lod_params(name, N, C, He, We, L, lod_stride, d, lod, pyramid, n_rows, p, T)) return 1;
    if (N == 0) dL_dlod = nullptr;  // (no row to write)
    const int go = rows_backward_prologue(name, N, grad_out, nullptr, dL_dd, dL_dlod != nullptr || dL_dpyramid != nullptr);
    if (go != SHADE_LAUNCH) return go;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (dL_dpyramid) {
        rows_fill_on(st, dL_dpyramid, T * C, 0u);
        if (launched(name)) return 1;
    }
    if (N == 0) return 0;
    const RowsGrid g = rows_grid(N, LOD_THREADS, LOD_MAX_GROUPS);
    const dim3 groups((unsigned)g.groups), block(LOD_THREADS);
    lod_with_wanted(dL_dd != nullptr, dL_dlod != nullptr, dL_dpyramid != nullptr, [&](auto wd, auto wl, auto wp) {  // (an output that is not wanted is null, and costs nothing)
        constexpr bool WD = decltype(wd)::value, WL = decltype(wl)::value, WP = decltype(wp)::value;
        k_envmap_lod_rows_backward<WD, WL, WP><<<groups, block, 0, st>>>(p, g.tiles, grad_out, dL_dd, dL_dlod, dL_dpyramid);
    });
    return launched(name);
}

#ifdef DMR_ABLATION
// (ablation build only) contributions to dL/dpyramid and those that left as direct atomics, since the last reset
int dmr_envmap_lod_stats(unsigned long long* out, int reset) {
    using namespace dmr;
    static const unsigned long long zeros[2] = {};
    if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(g_lod_stats), sizeof(zeros)) != hipSuccess) return api_fail("dmr_envmap_lod_stats: copy failed");
    if (reset && hipMemcpyToSymbol(HIP_SYMBOL(g_lod_stats), zeros, sizeof(zeros)) != hipSuccess) return api_fail("dmr_envmap_lod_stats: reset failed");
    return 0;
}
#endif

}  // extern "C"
