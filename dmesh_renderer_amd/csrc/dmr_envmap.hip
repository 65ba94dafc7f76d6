// dmr_envmap.hip -- direction rows looked up in a learnable lat-long environment map (include/dmesh_renderer_amd_envmap.h): the
// background between and behind the faces, and the specular term of packed rows fed a reflected direction; one forward and one
// backward kernel.  The model is fragments.envmap_rows:
//     n = |d[r]|   u = d / n (skipped when n is not finite or below 1e-8)   theta = acos(uz) = atan2(rho, uz)   phi = atan2(uy, ux)
//     x = (phi / 2 pi + 0.5) We - 0.5   y = (theta / pi) He - 0.5   x0 = floor(x), fx = x - x0 (likewise y)
//     y[r] = (1-fy) ((1-fx) env[iy0,ix0] + fx env[iy0,ix1]) + fy ((1-fx) env[iy1,ix0] + fx env[iy1,ix1]),  columns repeat, rows clamp
// A LANE OWNS A ROW: the four texel addresses and weights are formed once (env_coords, dmr_envmap_coords.hpp: plain C++ the CPU
// tests run on the host), then the channels go in chunks of four, as float4 texel reads when C % 4 == 0 and the map is 16-byte
// aligned.  y leaves either row by row, every lane its own, or through a per-wave LDS transpose so that consecutive lanes touch
// consecutive addresses -- per chunk count the shape that measured faster (profiles/envmap/store_shapes.txt; the ablation build's
// DMR_ABLATE bit ENV_OTHER_SHAPE runs the other one).  The backward's dL/dd re-reads the four texels and is a plain store per
// row; its dL/denvmap is a scatter-add that sums on chip what shares a destination before anything leaves, with the texture
// unit's machinery: the lanes of a wave that hold the same (texel, chunk) merge (shade_merge), the survivors add into a
// per-workgroup LDS table of f64 cells (stab_find_n), the table leaves as float atomics when more than half full and at the
// end, and what the table refuses goes out as direct atomics.
//
// Memory safety does not depend on the input bits: wrap_pair is the last step before the four indices, and every load, LDS key
// and atomic below takes its texel from there.  Rows r >= min(max(n_rows[0], 0), N) are not read.  Offsets into y, grad_out and
// the map are int64_t.
#include "dmr_rows_common.hpp"
#include "dmr_envmap_coords.hpp"
#include "../../include/dmesh_renderer_amd_envmap.h"

namespace dmr {
namespace {

#pragma clang fp contract(fast)

constexpr int ENV_THREADS = 256, ENV_MAX_GROUPS = DMR_ENVMAP_MAX_GROUPS, ENV_MAX_C = DMR_ENVMAP_MAX_CHANNELS;
// DMR_ABLATE bits of the ablation build (scripts/time_envmap.py): the other store shape of y; count what leaves as direct atomics
[[maybe_unused]] constexpr int ENV_OTHER_SHAPE = 1 << 26, ENV_STATS = 1 << 27;
// the shape of y's stores per chunk count (1, 2, 4: C <= 4, <= 8, <= 16): through the LDS transpose, or every lane its row.
// Measured per C (profiles/envmap/store_shapes.txt)
constexpr bool env_via_lds(int nch) { return nch >= 2; }
constexpr int env_pitch(int nch) { return (4 * nch) | 1; }  // (an odd row pitch: a wave's lanes on distinct banks)
constexpr size_t env_stage_bytes(int nch, bool via_lds) { return via_lds ? (size_t)(ENV_THREADS / 64) * 64 * env_pitch(nch) * sizeof(float) : 0; }
extern __shared__ __attribute__((aligned(16))) unsigned char env_lds[];
// The backward's table of texel gradients: keyed by texel x channel chunk, four f64 sums per cell; the scheme and the probe
// bound of dmr_shade_common.hpp at a size of its own: 36 KB of cells and keys, four workgroups per CU.
constexpr int ENV_TAB = 1024;
#ifdef DMR_ABLATION
__device__ unsigned long long g_env_stats[2];  // contributions to dL/denvmap (a row's texel x chunk), and those that left as direct atomics
#endif

struct EnvParams {
    int N, C, He, We;
    int nch;  // ceil(C / 4): channel chunks per texel
    int vec;  // a texel's chunk may be read as float4 (C % 4 == 0, 16-byte aligned base)
    const float* __restrict__ d;         // [N,3]
    const float* __restrict__ env;       // [He,We,C]
    const int32_t* __restrict__ n_rows;  // [1] or null
#ifdef DMR_ABLATION
    int dbg;
#endif
};

// A row as the kernels see it: whether it is used, the four texels (row-major indices into [He*We]: 00 = (iy0, ix0),
// 01 = (iy0, ix1), 10, 11) and the cell's fractions; what dL/dd needs beside them.
struct EnvRow {
    bool used, pole;
    uint32_t t[4];
    float fx, fy;
    float ux, uy, uz, inv, rho2;
};
__device__ __forceinline__ EnvRow env_row(const EnvParams& p, int64_t row, int n) {
    EnvRow r = {false, false, {0u, 0u, 0u, 0u}, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (row >= n) return r;
    const EnvCoords c = env_coords(p.d[row * 3], p.d[row * 3 + 1], p.d[row * 3 + 2], p.He, p.We);
    if (c.skipped) return r;
    r.used = true; r.pole = c.pole;
    const uint32_t r0 = (uint32_t)c.iy0 * (uint32_t)p.We, r1 = (uint32_t)c.iy1 * (uint32_t)p.We;
    r.t[0] = r0 + (uint32_t)c.ix0; r.t[1] = r0 + (uint32_t)c.ix1; r.t[2] = r1 + (uint32_t)c.ix0; r.t[3] = r1 + (uint32_t)c.ix1;
    r.fx = c.fx; r.fy = c.fy;
    r.ux = c.ux; r.uy = c.uy; r.uz = c.uz; r.inv = c.inv; r.rho2 = c.rho2;
    return r;
}

// channels c0 .. c0 + 3 of texel t (0 past C)
__device__ __forceinline__ void env_texel(const EnvParams& p, uint32_t t, int c0, float (&r)[4]) {
    const float* __restrict__ row = p.env + (int64_t)t * p.C + c0;
    if (p.vec) {
        const float4 v = *reinterpret_cast<const float4*>(row);
        r[0] = v.x; r[1] = v.y; r[2] = v.z; r[3] = v.w;
    } else {
#pragma unroll
        for (int c = 0; c < 4; c++) r[c] = c0 + c < p.C ? row[c] : 0.f;
    }
}

// ---------------------------------------------------------------------------
// forward.  A workgroup strides over tiles of 256 rows; a wave owns 64 consecutive rows and its own staging area, so there is
// no workgroup barrier.  NCH: the chunks of four channels a lane's registers hold (1, 2, 4: C <= 4, 8, 16; the chunk loop
// unrolled under uniform guards).  VIA_LDS: the wave's 64 rows of C floats go through its [64][4 NCH | 1] staging area and leave
// as 64 C consecutive floats, 256 bytes per store instruction; else every lane stores its own row.  A skipped row stores zeros.
// ---------------------------------------------------------------------------
template <int NCH, bool VIA_LDS>
__global__ void __launch_bounds__(ENV_THREADS)
k_envmap_rows(EnvParams p, int tiles, float* __restrict__ y) {
    constexpr int PITCH = env_pitch(NCH);
    const int tid = threadIdx.x, lane = tid & 63, C = p.C;
    [[maybe_unused]] float* st = reinterpret_cast<float*>(env_lds) + (tid >> 6) * (64 * PITCH);  // (VIA_LDS) the wave's staging area
    const int n = rows_used(p);
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t row = (int64_t)tile * ENV_THREADS + tid, row0 = row - lane;
        if (row0 >= p.N) continue;  // (wave-uniform)
        const EnvRow r = env_row(p, row, n);
        float o[4 * NCH];
#pragma unroll
        for (int c = 0; c < 4 * NCH; c++) o[c] = 0.f;
        if (r.used) {
            const float ax = 1.f - r.fx, ay = 1.f - r.fy;
            const float w00 = ay * ax, w01 = ay * r.fx, w10 = r.fy * ax, w11 = r.fy * r.fx;
#pragma unroll
            for (int i = 0; i < NCH; i++) {
                if (4 * i >= C) break;  // (uniform)
                float r0[4], r1[4], r2[4], r3[4];
                env_texel(p, r.t[0], 4 * i, r0); env_texel(p, r.t[1], 4 * i, r1);
                env_texel(p, r.t[2], 4 * i, r2); env_texel(p, r.t[3], 4 * i, r3);
#pragma unroll
                for (int j = 0; j < 4; j++) o[4 * i + j] = w00 * r0[j] + w01 * r1[j] + w10 * r2[j] + w11 * r3[j];
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
// backward.  A workgroup takes a contiguous run of row tiles: neighbouring rows (an image's pixels, a pack's slots) share
// texels, and stay in one workgroup's table.  Per row the four texels and the cell's fractions once; then per chunk of four
// channels
//   WD: e_i = texel_i . g of the four texels -> Gx += (1-fy)(e01 - e00) + fy (e11 - e10), Gy += (1-fx)(e10 - e00) + fx (e11 - e01);
//       then the chain of the header through (phi, theta) and the normalisation, one plain store per row (zeros in a skipped one
//       and at a pole);
//   WE: w_i g of the four texels, merged over the wave's lanes of equal (texel, chunk), into the table; a cell the table refuses
//       goes out with direct atomics.  After every tile the workgroup counts the table's keys and lets it leave when more than
//       half full; it leaves at the end.  Every lane of the workgroup runs every tile (merges, barriers).
// ---------------------------------------------------------------------------
template <bool WD, bool WE>
__global__ void __launch_bounds__(ENV_THREADS)
k_envmap_rows_backward(EnvParams p, int tiles, const float* __restrict__ gout, float* __restrict__ dd, float* __restrict__ denv) {
    __shared__ double tval[WE ? ENV_TAB : 1][4];
    __shared__ uint32_t tkey[WE ? ENV_TAB : 1];
    const int tid = threadIdx.x, lane = tid & 63, C = p.C;
    if constexpr (WE) {
        for (int i = tid; i < ENV_TAB; i += ENV_THREADS) {
            tkey[i] = STAB_EMPTY;
#pragma unroll
            for (int c = 0; c < 4; c++) tval[i][c] = 0.0;
        }
        __syncthreads();
    }
    // (between two barriers) every cell leaves, four lanes per cell -- a texel's chunk is 16 contiguous bytes --, and is empty again
    const auto flush = [&]() {
        for (int i = tid; i < ENV_TAB * 4; i += ENV_THREADS) {
            const uint32_t rid = tkey[i >> 2];
            if (rid == STAB_EMPTY) continue;
            const uint32_t t = rid / (uint32_t)p.nch;
            const int c = (int)(rid - t * (uint32_t)p.nch) * 4 + (i & 3);
            const double x = tval[i >> 2][i & 3];
            tval[i >> 2][i & 3] = 0.0;
            if (c < C && x != 0.0) unsafeAtomicAdd(&denv[(int64_t)t * C + c], (float)x);
        }
        __syncthreads();
        for (int i = tid; i < ENV_TAB; i += ENV_THREADS) tkey[i] = STAB_EMPTY;
    };
    const int n = rows_used(p);
    const RowsTileRun run = rows_tile_run(tiles);
    for (int tile = run.t0; tile < run.t1; tile++) {
        const int64_t row = (int64_t)tile * ENV_THREADS + tid;
        const EnvRow r = env_row(p, row, n);
        float out[3] = {0.f, 0.f, 0.f};
        if (__ballot(r.used) != 0ull) {  // (wave-uniform: the merge below runs with all 64 lanes)
            const float ax = 1.f - r.fx, ay = 1.f - r.fy;
            const float w[4] = {ay * ax, ay * r.fx, r.fy * ax, r.fy * r.fx};
            float Gx = 0.f, Gy = 0.f;
            for (int c0 = 0, ch = 0; c0 < C; c0 += 4, ch++) {  // (uniform)
                float g[4];
#pragma unroll
                for (int j = 0; j < 4; j++) g[j] = (r.used && c0 + j < C) ? gout[row * C + c0 + j] : 0.f;
                if constexpr (WD) {
                    if (r.used) {
                        float r0[4], r1[4], r2[4], r3[4];
                        env_texel(p, r.t[0], c0, r0); env_texel(p, r.t[1], c0, r1);
                        env_texel(p, r.t[2], c0, r2); env_texel(p, r.t[3], c0, r3);
                        float e0 = 0.f, e1 = 0.f, e2 = 0.f, e3 = 0.f;
#pragma unroll
                        for (int j = 0; j < 4; j++) { e0 += r0[j] * g[j]; e1 += r1[j] * g[j]; e2 += r2[j] * g[j]; e3 += r3[j] * g[j]; }
                        Gx += ay * (e1 - e0) + r.fy * (e3 - e2);
                        Gy += ax * (e2 - e0) + r.fx * (e3 - e1);
                    }
                }
                if constexpr (WE) {
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        const bool adds = r.used && w[i] != 0.f;
                        int key = adds ? (int)(r.t[i] * (uint32_t)p.nch + (uint32_t)ch) : -1;
                        float v[4];
#pragma unroll
                        for (int j = 0; j < 4; j++) v[j] = w[i] * g[j];
                        shade_merge(lane, key, v);
                        int slot = -1;
                        if (key >= 0) slot = stab_find_n<ENV_TAB>(tkey, (uint32_t)key);
                        if (key >= 0) {
#pragma unroll
                            for (int j = 0; j < 4; j++) {
                                if (c0 + j >= C) continue;
                                if (slot >= 0) atomicAdd(&tval[slot][j], (double)v[j]);
                                else unsafeAtomicAdd(&denv[(int64_t)r.t[i] * C + c0 + j], v[j]);
                            }
                        }
#ifdef DMR_ABLATION
                        if (DMR_DBG(p, ENV_STATS)) {
                            const unsigned long long all = __ballot(adds), direct = __ballot(key >= 0 && slot < 0);
                            if (lane == 0) { atomicAdd(&g_env_stats[0], (unsigned long long)__popcll(all)); atomicAdd(&g_env_stats[1], (unsigned long long)__popcll(direct)); }
                        }
#endif
                    }
                }
            }
            if constexpr (WD) {
                if (r.used && !r.pole) {
                    const float Gphi = Gx * ((float)p.We * ENV_INV_2PI), Gtheta = Gy * ((float)p.He * ENV_INV_PI);
                    const float ir2 = 1.f / r.rho2;
                    const float gx = -Gphi * r.uy * ir2, gy = Gphi * r.ux * ir2, gz = -Gtheta * sqrtf(ir2);
                    const float radial = r.ux * gx + r.uy * gy + r.uz * gz;
                    out[0] = (gx - r.ux * radial) * r.inv; out[1] = (gy - r.uy * radial) * r.inv; out[2] = (gz - r.uz * radial) * r.inv;
                }
            }
        }
        if constexpr (WD) {
            if (row < p.N) { dd[row * 3] = out[0]; dd[row * 3 + 1] = out[1]; dd[row * 3 + 2] = out[2]; }
        }
        if constexpr (WE) {
            int filled = 0;  // (uniform: every barrier below returns the workgroup's count)
            for (int i = tid; i < ENV_TAB; i += ENV_THREADS) filled += __syncthreads_count(tkey[i] != STAB_EMPTY);
            if (filled > ENV_TAB / 2) { flush(); __syncthreads(); }
        }
    }
    if constexpr (WE) { __syncthreads(); flush(); }
}

#pragma clang fp contract(off)

// what both calls check first, in the header's order -> EnvParams
int env_params(const char* name, int N, int C, int He, int We, const float* d, const float* envmap, const int32_t* n_rows, EnvParams& p) {
    const std::string n = std::string(name) + ": ";
    if (N < 0) return api_fail((n + "bad rows").c_str());
    if (C < 1 || C > ENV_MAX_C) return api_fail((n + "C must be in 1.." + std::to_string(ENV_MAX_C) + ", got " + std::to_string(C)).c_str());
    if (He < 1 || We < 1) return api_fail((n + "the map must have at least one texel").c_str());
    const int64_t nch = (C + 3) / 4;
    if ((int64_t)He * We * nch >= (int64_t)1 << 31) return api_fail((n + "map too large: He * We * ceil(C / 4) must be below 2^31").c_str());
    if (N > 0 && !d) return api_fail((n + "null d").c_str());
    if (N > 0 && !envmap) return api_fail((n + "null envmap").c_str());
    p.N = N; p.C = C; p.He = He; p.We = We;
    p.nch = (int)nch;
    p.vec = shade_vec(C, envmap);
    p.d = d; p.env = envmap; p.n_rows = n_rows;
#ifdef DMR_ABLATION
    p.dbg = ablate_bits();
#endif
    return 0;
}

}  // namespace
}  // namespace dmr

extern "C" {

int dmr_envmap_rows(int N, int C, int He, int We, const float* d, const float* envmap, const int32_t* n_rows, float* y, void* stream) {
    using namespace dmr;
    const char* name = "dmr_envmap_rows";
    EnvParams p;
    if (env_params(name, N, C, He, We, d, envmap, n_rows, p)) return 1;
    if (N == 0) return 0;
    if (!y) return api_fail("dmr_envmap_rows: null output");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const RowsGrid g = rows_grid(N, ENV_THREADS, ENV_MAX_GROUPS);
    const dim3 groups((unsigned)g.groups), block(ENV_THREADS);
    with_one_of<1, 2, 4>(p.nch, [&](auto nch) {  // (the 3 instantiations of the forward: C <= 4, <= 8, <= 16 -- 3 chunks run as 4)
        constexpr int NCH = decltype(nch)::value;
        constexpr bool L = env_via_lds(NCH);
#ifdef DMR_ABLATION
        if (ablate_bits() & ENV_OTHER_SHAPE) { k_envmap_rows<NCH, !L><<<groups, block, env_stage_bytes(NCH, !L), st>>>(p, g.tiles, y); return; }
#endif
        k_envmap_rows<NCH, L><<<groups, block, env_stage_bytes(NCH, L), st>>>(p, g.tiles, y);
    });
    return launched(name);
}

int dmr_envmap_rows_backward(int N, int C, int He, int We, const float* d, const float* envmap, const int32_t* n_rows,
                             const float* grad_out, float* dL_dd, float* dL_denvmap, void* stream) {
    using namespace dmr;
    const char* name = "dmr_envmap_rows_backward";
    EnvParams p;
    if (env_params(name, N, C, He, We, d, envmap, n_rows, p)) return 1;
    const int go = rows_backward_prologue(name, N, grad_out, nullptr, dL_dd, dL_denvmap != nullptr);
    if (go != SHADE_LAUNCH) return go;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (dL_denvmap) {
        rows_fill_on(st, dL_denvmap, (int64_t)He * We * C, 0u);
        if (launched(name)) return 1;
    }
    if (N == 0) return 0;
    const RowsGrid g = rows_grid(N, ENV_THREADS, ENV_MAX_GROUPS);
    const dim3 groups((unsigned)g.groups), block(ENV_THREADS);
    with_wanted(dL_dd != nullptr, dL_denvmap != nullptr, [&](auto wd, auto we) {  // (the 3 of the backward: an output that is not wanted is null, and its kernel has no table)
        constexpr bool WD = decltype(wd)::value, WE = decltype(we)::value;
        k_envmap_rows_backward<WD, WE><<<groups, block, 0, st>>>(p, g.tiles, grad_out, dL_dd, dL_denvmap);
    });
    return launched(name);
}

#ifdef DMR_ABLATION
// (ablation build only) contributions to dL/denvmap and those that left as direct atomics, since the last reset
int dmr_envmap_stats(unsigned long long* out, int reset) {
    using namespace dmr;
    static const unsigned long long zeros[2] = {};
    if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(g_env_stats), sizeof(zeros)) != hipSuccess) return api_fail("dmr_envmap_stats: copy failed");
    if (reset && hipMemcpyToSymbol(HIP_SYMBOL(g_env_stats), zeros, sizeof(zeros)) != hipSuccess) return api_fail("dmr_envmap_stats: reset failed");
    return 0;
}
#endif

}  // extern "C"
