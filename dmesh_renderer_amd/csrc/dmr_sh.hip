// dmr_sh.hip -- the view direction of packed rows as a real spherical-harmonics encoding (include/dmesh_renderer_amd_sh.h): the
// second input of dmr_mlp.hip's MLP beside dmr_hashgrid.hip's field, one forward and one backward kernel, and the map from a
// packed row to its view (dmr_packed_row_views).  The models are fragments.sh_rows and fragments.packed_row_views:
//     v = row_view[r] (or 0)   w = x[r] - origin[v] (or x[r])   n = |w|   d = w / n (0 when n is not finite or below 1e-8)
//     y[r, l l + l + m] = Y_lm(d)                                          (degree^2 channels, homogeneous polynomials of d)
//     dL/dw = (gd - d (d . gd)) / n with gd = sum_i g_i dY_i/dd;   dL/dx[r] = dL/dw;   dL/dorigin[v] = - sum_r dL/dw
// A LANE OWNS A ROW; `degree` is a template parameter, so a row's up to 16 channels are registers.  y leaves (and grad_out
// arrives) either row by row, every lane its own, or through a per-wave LDS transpose so that consecutive lanes touch
// consecutive addresses -- per degree and direction the shape that measured faster: y transposed at degree 3 and 4, grad_out
// row by row at every degree (profiles/sh/store_shapes.txt; the ablation build's DMR_ABLATE bit SH_OTHER_SHAPE runs the other one).  dL/dorigin sums on chip: a wave whose rows are of one view reduces its
// three values with DPP and adds once into the workgroup's LDS table of f64 cells [B][3], a mixed wave adds per lane; the table
// leaves once per workgroup with one float atomic per non-zero cell.
//
// Rows r >= min(max(n_rows[0], 0), N) and rows whose view lies outside [0, B) are not read.  Offsets into y and grad_out are
// int64_t.
#include <cfloat>

#include "dmr_deferred_common.hpp"
#include "dmr_rows_common.hpp"
#include "../../include/dmesh_renderer_amd_sh.h"

namespace dmr {
namespace {

#pragma clang fp contract(fast)

constexpr int SH_THREADS = 256, SH_MAX_GROUPS = DMR_SH_MAX_GROUPS, SH_MAX_VIEWS = DMR_SH_MAX_VIEWS;
constexpr int SH_OTHER_SHAPE = 1 << 25;  // DMR_ABLATE bit of the ablation build (scripts/time_sh.py): the other store / load shape
// the shape of y's stores and of grad_out's loads per degree (1, 4, 9, 16 channels): through the LDS transpose, or every lane its
// row.  Measured per degree (profiles/sh/store_shapes.txt): the stores of 9 and 16 channels are faster transposed, the loads never
constexpr bool sh_via_lds(int degree) { return degree >= 3; }
constexpr bool sh_loads_via_lds(int) { return false; }
constexpr int sh_pitch(int c) { return c | 1; }  // (an odd row pitch: a wave's lanes on distinct banks)
// All LDS of both kernels is the launch's dynamic region, 16-byte aligned: the backward's table of f64 cells first (24 B bytes,
// rounded up to 16), then the transpose's staging area of 64 rows per wave.  No static LDS in front of it: that would shift the
// f64 cells off their alignment.
constexpr size_t sh_stage_bytes(int degree, bool via_lds) { return via_lds ? (size_t)(SH_THREADS / 64) * 64 * sh_pitch(degree * degree) * sizeof(float) : 0; }
inline size_t sh_table_bytes(int B) { return ((size_t)3 * B * sizeof(double) + 15) & ~(size_t)15; }
extern __shared__ __attribute__((aligned(16))) unsigned char sh_lds[];

struct ShParams {
    int N, B;
    const float* __restrict__ x;            // [N,3]
    const float* __restrict__ origin;       // [B,3] or null: x holds w
    const int32_t* __restrict__ row_view;   // [N] or null: view 0
    const int32_t* __restrict__ n_rows;     // [1] or null
};

// a row as the kernels see it: whether it is read at all, its view, its direction and 1 / n (0 with a zero direction)
struct ShRow {
    bool active;
    int v;
    float x, y, z, inv;
};
__device__ __forceinline__ ShRow sh_row(const ShParams& p, int64_t row, int n) {
    ShRow r = {row < n, 0, 0.f, 0.f, 0.f, 0.f};
    if (r.active && p.row_view) {
        r.v = p.row_view[row];
        r.active = (uint32_t)r.v < (uint32_t)p.B;
    }
    if (!r.active) { r.v = 0; return r; }
    float wx = p.x[row * 3], wy = p.x[row * 3 + 1], wz = p.x[row * 3 + 2];
    if (p.origin) { wx -= p.origin[r.v * 3]; wy -= p.origin[r.v * 3 + 1]; wz -= p.origin[r.v * 3 + 2]; }
    const float len = sqrtf(wx * wx + wy * wy + wz * wz);
    const bool ok = len >= 1e-8f && len <= FLT_MAX;  // (false for NaN)
    r.inv = ok ? 1.f / len : 0.f;
    r.x = ok ? wx * r.inv : 0.f; r.y = ok ? wy * r.inv : 0.f; r.z = ok ? wz * r.inv : 0.f;
    return r;
}

// the table of the header, channel l l + l + m
constexpr float SH_C0 = 0.28209479177387814f, SH_C1 = 0.4886025119029199f;
constexpr float SH_C2A = 1.0925484305920792f, SH_C2B = 0.31539156525252005f, SH_C2C = 0.5462742152960396f;
constexpr float SH_C3A = 0.5900435899266435f, SH_C3B = 2.890611442640554f, SH_C3C = 0.4570457994644658f, SH_C3D = 0.3731763325901154f,
                SH_C3E = 1.445305721320277f;

template <int DEG>
__device__ __forceinline__ void sh_eval(float x, float y, float z, float (&o)[DEG * DEG]) {
    o[0] = SH_C0;
    if constexpr (DEG >= 2) { o[1] = -SH_C1 * y; o[2] = SH_C1 * z; o[3] = -SH_C1 * x; }
    if constexpr (DEG >= 3) {
        const float xx = x * x, yy = y * y, zz = z * z;
        o[4] = SH_C2A * (x * y); o[5] = -SH_C2A * (y * z); o[6] = SH_C2B * (2.f * zz - xx - yy); o[7] = -SH_C2A * (x * z);
        o[8] = SH_C2C * (xx - yy);
        if constexpr (DEG >= 4) {
            o[9] = -SH_C3A * y * (3.f * xx - yy); o[10] = SH_C3B * (x * y) * z; o[11] = -SH_C3C * y * (4.f * zz - xx - yy);
            o[12] = SH_C3D * z * (2.f * zz - 3.f * xx - 3.f * yy); o[13] = -SH_C3C * x * (4.f * zz - xx - yy);
            o[14] = SH_C3E * z * (xx - yy); o[15] = -SH_C3A * x * (xx - 3.f * yy);
        }
    }
}

// gd = sum_i g_i dY_i/dd, the polynomials' derivative as functions of a free vector
template <int DEG>
__device__ __forceinline__ void sh_grad(float x, float y, float z, const float (&g)[DEG * DEG], float& gx, float& gy, float& gz) {
    gx = 0.f; gy = 0.f; gz = 0.f;
    if constexpr (DEG >= 2) { gy = -SH_C1 * g[1]; gz = SH_C1 * g[2]; gx = -SH_C1 * g[3]; }
    if constexpr (DEG >= 3) {
        gx += SH_C2A * (g[4] * y - g[7] * z) + 2.f * x * (SH_C2C * g[8] - SH_C2B * g[6]);
        gy += SH_C2A * (g[4] * x - g[5] * z) - 2.f * y * (SH_C2C * g[8] + SH_C2B * g[6]);
        gz += 4.f * SH_C2B * g[6] * z - SH_C2A * (g[5] * y + g[7] * x);
    }
    if constexpr (DEG >= 4) {
        const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, xz = x * z, yz = y * z;
        gx += -6.f * SH_C3A * g[9] * xy + SH_C3B * g[10] * yz + 2.f * SH_C3C * g[11] * xy - 6.f * SH_C3D * g[12] * xz
              - SH_C3C * g[13] * (4.f * zz - 3.f * xx - yy) + 2.f * SH_C3E * g[14] * xz - 3.f * SH_C3A * g[15] * (xx - yy);
        gy += -3.f * SH_C3A * g[9] * (xx - yy) + SH_C3B * g[10] * xz - SH_C3C * g[11] * (4.f * zz - xx - 3.f * yy) - 6.f * SH_C3D * g[12] * yz
              + 2.f * SH_C3C * g[13] * xy - 2.f * SH_C3E * g[14] * yz + 6.f * SH_C3A * g[15] * xy;
        gz += SH_C3B * g[10] * xy - 8.f * SH_C3C * g[11] * yz + 3.f * SH_C3D * g[12] * (2.f * zz - xx - yy) - 8.f * SH_C3C * g[13] * xz
              + SH_C3E * g[14] * (xx - yy);
    }
}

// ---------------------------------------------------------------------------
// forward.  A workgroup strides over tiles of 256 rows; a wave owns 64 consecutive rows and its own staging area, so there is
// no workgroup barrier.  VIA_LDS: the wave's 64 rows of C floats go through its [64][C | 1] staging area and leave as 64 C
// consecutive floats, 256 bytes per store instruction; else every lane stores its own row.  A skipped row stores zeros.
// ---------------------------------------------------------------------------
template <int DEG, bool VIA_LDS>
__global__ void __launch_bounds__(SH_THREADS)
k_sh_rows(ShParams p, int tiles, float* __restrict__ y) {
    constexpr int C = DEG * DEG, PITCH = sh_pitch(C);
    const int tid = threadIdx.x, lane = tid & 63;
    [[maybe_unused]] float* st = reinterpret_cast<float*>(sh_lds) + (tid >> 6) * (64 * PITCH);  // (VIA_LDS) the wave's staging area
    const int n = rows_used(p);
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t row = (int64_t)tile * SH_THREADS + tid, row0 = row - lane;
        if (row0 >= p.N) continue;  // (wave-uniform)
        const ShRow r = sh_row(p, row, n);
        float o[C];
        sh_eval<DEG>(r.x, r.y, r.z, o);
        if (!r.active) {
#pragma unroll
            for (int c = 0; c < C; c++) o[c] = 0.f;
        }
        if constexpr (VIA_LDS) {
#pragma unroll
            for (int c = 0; c < C; c++) st[lane * PITCH + c] = o[c];
            rows_wave_sync();
            const int64_t left = ((int64_t)p.N - row0) * C;  // the floats of y from the wave's first row on
#pragma unroll
            for (int i = 0; i < C; i++) {
                const int e = i * 64 + lane;
                if (e < left) y[row0 * C + e] = st[(e / C) * PITCH + e % C];
            }
            rows_wave_sync();
        } else if (row < p.N) {
#pragma unroll
            for (int c = 0; c < C; c++) y[row * C + c] = o[c];
        }
    }
}

// ---------------------------------------------------------------------------
// backward.  A workgroup takes a contiguous run of row tiles (rows are numbered view-major: a workgroup then meets one view,
// seldom two).  WX: dL/dx, a plain store per row (zeros in a skipped one).  WO: dL/dorigin through the workgroup's table.
// VIA_LDS (the ablation build's other shape): grad_out arrives as 64 C consecutive floats per wave and is transposed in LDS; else
// every lane loads its own row.
// ---------------------------------------------------------------------------
template <int CTRL>
__device__ __forceinline__ float sh_dpp(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}
// the sum of v over the wave's 64 lanes, in every lane (called by all 64): quad_perm [1,0,3,2], [2,3,0,1], row_half_mirror,
// row_mirror give every lane its 16-lane row's sum; the four rows' sums are read across
__device__ __forceinline__ float sh_wave_sum(float v) {
    v += sh_dpp<0xB1>(v);
    v += sh_dpp<0x4E>(v);
    v += sh_dpp<0x141>(v);
    v += sh_dpp<0x140>(v);
    const int b = __float_as_int(v);
    return (__int_as_float(__builtin_amdgcn_readlane(b, 0)) + __int_as_float(__builtin_amdgcn_readlane(b, 16))) +
           (__int_as_float(__builtin_amdgcn_readlane(b, 32)) + __int_as_float(__builtin_amdgcn_readlane(b, 48)));
}

template <int DEG, bool WX, bool WO, bool VIA_LDS>
__global__ void __launch_bounds__(SH_THREADS)
k_sh_rows_backward(ShParams p, int tiles, int lds_table, const float* __restrict__ gout, float* __restrict__ dx, float* __restrict__ dorigin) {
    constexpr int C = DEG * DEG, PITCH = sh_pitch(C);
    const int tid = threadIdx.x, lane = tid & 63;
    [[maybe_unused]] double* tab = reinterpret_cast<double*>(sh_lds);  // (WO) [B][3]
    [[maybe_unused]] float* st = reinterpret_cast<float*>(sh_lds + (WO ? lds_table : 0)) + (tid >> 6) * (64 * PITCH);  // (VIA_LDS)
    if constexpr (WO) {
        for (int i = tid; i < 3 * p.B; i += SH_THREADS) tab[i] = 0.0;
        __syncthreads();
    }
    const int n = rows_used(p);
    const RowsTileRun run = rows_tile_run(tiles);
    for (int tile = run.t0; tile < run.t1; tile++) {
        const int64_t row = (int64_t)tile * SH_THREADS + tid, row0 = row - lane;
        if (row0 >= p.N) continue;  // (wave-uniform)
        const ShRow r = sh_row(p, row, n);
        const unsigned long long live = __ballot(r.active);
        float d[3] = {0.f, 0.f, 0.f};
        if (live != 0ull) {  // (wave-uniform: the transpose and the wave's sum run with all 64 lanes)
            float g[C];
            if constexpr (VIA_LDS) {
                const int64_t left = ((int64_t)p.N - row0) * C;
#pragma unroll
                for (int i = 0; i < C; i++) {
                    const int e = i * 64 + lane;
                    st[(e / C) * PITCH + e % C] = e < left ? gout[row0 * C + e] : 0.f;
                }
                rows_wave_sync();
#pragma unroll
                for (int c = 0; c < C; c++) g[c] = st[lane * PITCH + c];
                rows_wave_sync();
            } else {
#pragma unroll
                for (int c = 0; c < C; c++) g[c] = r.active ? gout[row * C + c] : 0.f;
            }
            if (r.active) {  // (a skipped row's g may hold anything: it is not used)
                float gx, gy, gz;
                sh_grad<DEG>(r.x, r.y, r.z, g, gx, gy, gz);
                const float radial = r.x * gx + r.y * gy + r.z * gz;
                d[0] = (gx - r.x * radial) * r.inv; d[1] = (gy - r.y * radial) * r.inv; d[2] = (gz - r.z * radial) * r.inv;
                if (r.inv == 0.f) { d[0] = 0.f; d[1] = 0.f; d[2] = 0.f; }  // (a zero direction: an exact 0 whatever g holds)
            }
            if constexpr (WO) {
                const int v0 = __shfl(r.v, __ffsll(live) - 1);
                if (__ballot(r.active && r.v != v0) == 0ull) {  // (wave-uniform) one view: one add per value
                    const float s0 = sh_wave_sum(d[0]), s1 = sh_wave_sum(d[1]), s2 = sh_wave_sum(d[2]);
                    if (lane == 0) {
                        atomicAdd(&tab[3 * v0], -(double)s0); atomicAdd(&tab[3 * v0 + 1], -(double)s1); atomicAdd(&tab[3 * v0 + 2], -(double)s2);
                    }
                } else if (r.active) {
                    atomicAdd(&tab[3 * r.v], -(double)d[0]); atomicAdd(&tab[3 * r.v + 1], -(double)d[1]); atomicAdd(&tab[3 * r.v + 2], -(double)d[2]);
                }
            }
        }
        if constexpr (WX) {
            if (row < p.N) { dx[row * 3] = d[0]; dx[row * 3 + 1] = d[1]; dx[row * 3 + 2] = d[2]; }
        }
    }
    if constexpr (WO) {
        __syncthreads();
        for (int i = tid; i < 3 * p.B; i += SH_THREADS) {
            const double s = tab[i];
            if (s != 0.0) unsafeAtomicAdd(&dorigin[i], (float)s);
        }
    }
}

// ---------------------------------------------------------------------------
// the view of every packed row: one walk of the slots on the packed unit's row-shaped lanes (RowPix: a wave on 64 pixels of an
// image row), k by k -- 64 consecutive slots of the flattened lists per load.  A slot with 0 <= row < N writes its view.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_sh_row_views(int B, int K, int H, int W, int N, int sx, int sy, const int32_t* __restrict__ row, int32_t* __restrict__ view_out) {
    const RowPix S((int)blockIdx.x, sx, sy, W, H);
    if (!S.inside) return;
    for (int k = 0; k < K; k++) {
        const int r = row[((int64_t)S.b * K + k) * S.HW + S.pix];
        if ((uint32_t)r < (uint32_t)N) view_out[r] = S.b;
    }
}

#pragma clang fp contract(off)

// what both encoding calls check first, in the header's order -> ShParams
int sh_params(const char* name, int N, int degree, int B, const float* x, const float* origin, const int32_t* row_view, const int32_t* n_rows,
              ShParams& p) {
    const std::string n = std::string(name) + ": ";
    if (N < 0) return api_fail((n + "bad rows").c_str());
    if (degree < 1 || degree > DMR_SH_MAX_DEGREE) return api_fail((n + "degree must be in 1..4, got " + std::to_string(degree)).c_str());
    if (row_view && !origin) return api_fail((n + "row_view without origin").c_str());
    if (origin && (B < 1 || B > SH_MAX_VIEWS)) return api_fail((n + "B must be in 1.." + std::to_string(SH_MAX_VIEWS) + ", got " + std::to_string(B)).c_str());
    if (N > 0 && !x) return api_fail((n + "null x").c_str());
    p.N = N; p.B = origin ? B : 1;
    p.x = x; p.origin = origin; p.row_view = row_view; p.n_rows = n_rows;
    return 0;
}

}  // namespace
}  // namespace dmr

extern "C" {

int dmr_packed_row_views(int B, int K, int H, int W, int N, const int32_t* row, int32_t* view_out, void* stream) {
    using namespace dmr;
    const char* name = "dmr_packed_row_views";
    const std::string n = std::string(name) + ": ";
    if (B < 0 || H < 0 || W < 0 || N < 0) return api_fail((n + "bad dimensions").c_str());
    if (K < 1 || K > 32) return api_fail((n + "K must be in 1..32, got " + std::to_string(K)).c_str());
    const int64_t sx = (W + ROW_W - 1) / ROW_W, sy = (H + ROW_H - 1) / ROW_H;
    if ((int64_t)B * K * H * W >= (int64_t)1 << 31 || (int64_t)B * sx * sy >= (int64_t)1 << 31) return api_fail((n + "problem too large").c_str());
    const bool slots = (int64_t)B * H * W > 0;
    if (slots && !row) return api_fail((n + "null row").c_str());
    if (N > 0 && !view_out) return api_fail((n + "null output").c_str());
    if (N == 0 || !slots) return 0;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    rows_fill_on(st, view_out, N, 0xffffffffu);
    if (launched(name)) return 1;
    k_sh_row_views<<<dim3((unsigned)(B * sx * sy)), dim3(256), 0, st>>>(B, K, H, W, N, (int)sx, (int)sy, row, view_out);
    return launched(name);
}

int dmr_sh_rows(int N, int degree, int B, const float* x, const float* origin, const int32_t* row_view, const int32_t* n_rows,
                float* y, void* stream) {
    using namespace dmr;
    const char* name = "dmr_sh_rows";
    ShParams p;
    if (sh_params(name, N, degree, B, x, origin, row_view, n_rows, p)) return 1;
    if (N == 0) return 0;
    if (!y) return api_fail("dmr_sh_rows: null output");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const RowsGrid g = rows_grid(N, SH_THREADS, SH_MAX_GROUPS);
    const dim3 groups((unsigned)g.groups), block(SH_THREADS);
    with_one_of<1, 2, 3, 4>(degree, [&](auto deg) {  // (the 4 instantiations of the forward)
        constexpr int D = decltype(deg)::value;
        constexpr bool L = sh_via_lds(D);
#ifdef DMR_ABLATION
        if (ablate_bits() & SH_OTHER_SHAPE) { k_sh_rows<D, !L><<<groups, block, sh_stage_bytes(D, !L), st>>>(p, g.tiles, y); return; }
#endif
        k_sh_rows<D, L><<<groups, block, sh_stage_bytes(D, L), st>>>(p, g.tiles, y);
    });
    return launched(name);
}

int dmr_sh_rows_backward(int N, int degree, int B, const float* x, const float* origin, const int32_t* row_view,
                         const int32_t* n_rows, const float* grad_out, float* dL_dx, float* dL_dorigin, void* stream) {
    using namespace dmr;
    const char* name = "dmr_sh_rows_backward";
    ShParams p;
    if (sh_params(name, N, degree, B, x, origin, row_view, n_rows, p)) return 1;
    const int go = rows_backward_prologue(name, N, grad_out, dL_dorigin && !origin ? "dL_dorigin without origin" : nullptr, dL_dx, dL_dorigin != nullptr);
    if (go != SHADE_LAUNCH) return go;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (dL_dorigin) {
        rows_fill_on(st, dL_dorigin, (int64_t)3 * B, 0u);
        if (launched(name)) return 1;
    }
    if (N == 0) return 0;
    const RowsGrid g = rows_grid(N, SH_THREADS, SH_MAX_GROUPS);
    const dim3 groups((unsigned)g.groups), block(SH_THREADS);
    const size_t tab = sh_table_bytes(p.B);  // the workgroup's table of dL/dorigin
    with_one_of<1, 2, 3, 4>(degree, [&](auto deg) {  // (... the 12 of the backward)
        constexpr int D = decltype(deg)::value;
        constexpr bool L = sh_loads_via_lds(D);
        with_wanted(dL_dx != nullptr, dL_dorigin != nullptr, [&](auto wx, auto wo) {  // (an output that is not wanted is null, and its kernel has no table)
            constexpr bool WX = decltype(wx)::value, WO = decltype(wo)::value;
            const size_t table = WO ? tab : 0;
#ifdef DMR_ABLATION
            if (ablate_bits() & SH_OTHER_SHAPE) { k_sh_rows_backward<D, WX, WO, !L><<<groups, block, table + sh_stage_bytes(D, !L), st>>>(p, g.tiles, (int)table, grad_out, dL_dx, dL_dorigin); return; }
#endif
            k_sh_rows_backward<D, WX, WO, L><<<groups, block, table + sh_stage_bytes(D, L), st>>>(p, g.tiles, (int)table, grad_out, dL_dx, dL_dorigin);
        });
    });
    return launched(name);
}

}  // extern "C"
