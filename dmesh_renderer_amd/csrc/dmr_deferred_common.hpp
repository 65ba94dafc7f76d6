// dmr_deferred_common.hpp -- what the deferred shading units (dmr_interp.hip on [B,K,C,H,W] planes, dmr_packed.hip on [N,C] rows)
// share, each fact once, on top of dmr_shade_common.hpp:
//   device: the two pixel-to-lane mappings (RowPix, TilePix), the backward kernels' LDS tables (InterpLds, ValuesLds), the vertex
//           lookup (interp_verts) and the zeroing kernel (k_deferred_zero / zero_on), which dmr_visibility.hip launches too;
//   host:   the grids (deferred_grids), the parameter blocks both calls of a pair fill (deferred_interp_params,
//           deferred_values_params) and what a composite_values*_backward call does before it launches (values_backward_prologue).
// The packed unit's extra list arguments arrive as a PackedRows (null: the dense unit), its checks at the places they had.
// The kernels' walks stay each unit's own text, and so does the dense unit's row load: shared formulations of either change the
// kernels' code.
#pragma once

#include "dmr_shade_common.hpp"

namespace dmr {
namespace {

// The streaming kernels' mapping: a 256-thread workgroup on ROW_W x ROW_H pixels, each wave on one row of them.
constexpr int ROW_W = 64, ROW_H = 4;
struct RowPix {
    int px, py, b;
    bool inside;
    int64_t HW, pix;
    __device__ __forceinline__ RowPix(int block, int sx, int sy, int W, int H) {
        px = (block % sx) * ROW_W + (int)(threadIdx.x & 63); py = ((block / sx) % sy) * ROW_H + (int)(threadIdx.x >> 6);
        b = block / (sx * sy);
        inside = px < W && py < H;
        HW = (int64_t)H * W;
        pix = (int64_t)W * py + px;
    }
    template <class P> __host__ __device__ static int nx(const P& p) { return p.sx; }
    template <class P> __host__ __device__ static int ny(const P& p) { return p.sy; }
};
// The fragment kernels' mapping (FragSlots) with RowPix's members: a workgroup on a 16 x 16 tile, 8 x 8 pixels per wave.
struct TilePix {
    int b;
    bool inside;
    int64_t HW, pix;
    __device__ __forceinline__ TilePix(int block, int gx, int gy, int W, int H) {
        const auto [tx, ty, view] = tile_coords(block, gx, gy);
        const FragSlots S(tx, ty, view, 1, W, H);
        b = view; inside = S.inside; HW = S.HW;
        pix = (int64_t)W * S.py + S.px;
    }
    template <class P> __host__ __device__ static int nx(const P& p) { return p.gx; }
    template <class P> __host__ __device__ static int ny(const P& p) { return p.gy; }
};
// Which of the two a backward kernel runs on: both merge lanes of equal face inside 16-lane DPP rows -- 16 x 1 pixels under
// RowPix, 8 x 2 under TilePix -- and sum per workgroup; chosen per kernel by measurement, for both units.
using InterpBackwardPix = TilePix;
using ValuesBackwardPix = RowPix;

// The three vertices of a face; false when one of them is no row of vert_attrs (such a slot gathers and scatters nothing).
template <class P>
__device__ __forceinline__ bool interp_verts(const P& p, int face, int (&v)[3]) {
    v[0] = p.faces[3 * face]; v[1] = p.faces[3 * face + 1]; v[2] = p.faces[3 * face + 2];
    return (uint32_t)v[0] < (uint32_t)p.P && (uint32_t)v[1] < (uint32_t)p.P && (uint32_t)v[2] < (uint32_t)p.P;
}

// The interpolation backward's per-tile table: vertex -> CH sums in f64 cells (as the other units' tables: an f64 LDS add on
// distinct cells costs a tenth of an f32 one on this part, profiles/r02/lds_atomics.txt): 20 KB (CH 4), 38 KB (CH 8).
template <int CH>
struct InterpLds {
    double val[STAB][CH];
    uint32_t key[STAB];
};
// The blend backward's: T_k and e_k = values_k . g of every slot of the workgroup's pixels (what the opacity recurrence needs
// from the front-to-back walk), and the table: face -> (dL/do, dL/ds) in f64 cells.
// 8 KB + 11 KB (KMAX 4) ... 64 KB + 11 KB (KMAX 32).
template <int KMAX>
struct ValuesLds {
    float tv[KMAX][TILE_PIX];
    float ev[KMAX][TILE_PIX];
    double val[STAB][2];
    uint32_t key[STAB];
};

// Up to three buffers of 4-byte words zeroed by one launch (null: none), each with its own length: what the tiles add into, and
// dL/dvalues when no upstream of the image arrives.  A kernel, not hipMemsetAsync: that is a fill kernel per buffer, and as a
// node of a captured graph it left small non-zero words behind from the second replay on.
__global__ void __launch_bounds__(256)
k_deferred_zero(uint32_t* __restrict__ a, int64_t na, uint32_t* __restrict__ b, int64_t nb, uint32_t* __restrict__ c, int64_t nc) {
    const int64_t step = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; (a && i < na) || (b && i < nb) || (c && i < nc); i += step) {
        if (a && i < na) a[i] = 0u;
        if (b && i < nb) b[i] = 0u;
        if (c && i < nc) c[i] = 0u;
    }
}
constexpr int64_t ZERO_MAX_BLOCKS = 1 << 16;  // (a grid stride beyond: B K C H W words may pass what one grid dimension holds)
void zero_on(hipStream_t st, void* a, int64_t na, void* b, int64_t nb, void* c, int64_t nc) {
    int64_t n = 0;
    if (a && na > n) n = na;
    if (b && nb > n) n = nb;
    if (c && nc > n) n = nc;
    if (n <= 0) return;
    const int64_t blocks = (n + 255) / 256;
    k_deferred_zero<<<dim3((unsigned)(blocks < ZERO_MAX_BLOCKS ? blocks : ZERO_MAX_BLOCKS)), dim3(256), 0, st>>>(
        static_cast<uint32_t*>(a), na, static_cast<uint32_t*>(b), nb, static_cast<uint32_t*>(c), nc);
}

// ---- Host side.  (Neither pair fits shade_check_lists: one has no opacities, the other no barycentrics and no corner table.)
// What the packed calls pass beside the dense ones' lists: N rows, row [B,K,H,W], n_used [1].
struct PackedRows { int N; const int32_t* row; const int32_t* n_used; };

// The grids of both mappings -> the fields of the unit's parameter block; non-zero with the error set.  tail_groups: the
// workgroups a launch adds past the grid's own; slots: what the unit indexes with 32 bits (K H W dense, B K H W packed).
template <class P>
int deferred_grids(const std::string& n, int B, int K, int H, int W, int F, int C, int tail_groups, int64_t slots, P& p) {
    const int64_t gx = (W + TILE - 1) / TILE, gy = (H + TILE - 1) / TILE;
    const int64_t sx = (W + ROW_W - 1) / ROW_W, sy = (H + ROW_H - 1) / ROW_H;
    if ((int64_t)B * gx * gy + tail_groups >= (int64_t)1 << 31 || (int64_t)B * sx * sy + tail_groups >= (int64_t)1 << 31 ||
        (int64_t)B * F >= (int64_t)1 << 31 || slots >= (int64_t)1 << 31)
        return api_fail((n + "problem too large").c_str());
    p.B = B; p.K = K; p.H = H; p.W = W; p.F = F; p.C = C; p.gx = (int)gx; p.gy = (int)gy; p.sx = (int)sx; p.sy = (int)sy;
    return 0;
}

// the arguments both interpolate calls of a unit share -> its parameter block (a packed unit sets N, row and n_used itself)
template <class P>
int deferred_interp_params(const char* name, int max_c, int B, int K, int H, int W, int Pn, int F, int C, const int32_t* face,
                           const float* bary, const int32_t* faces, const float* vert_attrs, const PackedRows* r, int tail_groups,
                           int64_t slots, P& p) {
    const std::string n = std::string(name) + ": ";
    if (shade_check_sizes(n, B, K, H, W, Pn, F, C, max_c)) return 1;
    if (r && r->N < 0) return api_fail((n + "bad rows").c_str());
    if (!face || !bary || (r && !r->row)) return api_fail((n + "null fragment lists").c_str());
    if (F > 0 && !faces) return api_fail((n + "null faces").c_str());
    if (F > 0 && Pn > 0 && !vert_attrs) return api_fail((n + "null vert_attrs").c_str());
    if (r && !r->n_used) return api_fail((n + "null n_used").c_str());
    if (deferred_grids(n, B, K, H, W, F, C, tail_groups, slots, p)) return 1;
    p.P = Pn;
    p.vec = shade_vec(C, vert_attrs);
    p.face = face; p.bary = bary; p.faces = faces; p.attrs = vert_attrs;
    return 0;
}

// the arguments both composite_values calls of a unit share -> its parameter block (values may be null where there is no row)
template <class P>
int deferred_values_params(const char* name, int max_c, int B, int K, int H, int W, int F, int C, const int32_t* face,
                           const float* faces_opacity, const float* values, const float* face_scale, const PackedRows* r,
                           int tail_groups, int64_t slots, P& p) {
    const std::string n = std::string(name) + ": ";
    if (shade_check_sizes(n, B, K, H, W, 0, F, C, max_c)) return 1;
    if (r && r->N < 0) return api_fail((n + "bad rows").c_str());
    if (!face || (r && !r->row)) return api_fail((n + "null fragment lists").c_str());
    if (F > 0 && !faces_opacity) return api_fail((n + "null faces_opacity").c_str());
    if ((!r || r->N > 0) && !values) return api_fail((n + "null values").c_str());
    if (deferred_grids(n, B, K, H, W, F, C, tail_groups, slots, p)) return 1;
    p.face = face; p.opacity = faces_opacity; p.values = values; p.scale = face_scale;
    return 0;
}

// What a composite_values*_backward call does between its checks and its launch: what the workgroups add into is zeroed, and
// dL/dvalues (n_values floats) when no upstream of the image arrives -- the kernel does not store it then.  -> SHADE_LAUNCH with
// the kernel's three outputs (null: not wanted, or nothing to add), SHADE_DONE (the zeros are the gradients) or SHADE_FAILED.
inline int values_backward_prologue(const char* name, hipStream_t st, int B, int F, int64_t n_values, const float* grad_image,
                                    const float* grad_T, float* dL_dfaces_opacity, float* dL_dvalues, float* dL_dface_scale,
                                    float*& dop, float*& dval, float*& dsc) {
    zero_on(st, dL_dfaces_opacity, F, dL_dface_scale, (int64_t)B * F, grad_image ? nullptr : dL_dvalues, n_values);
    if (launched(name)) return SHADE_FAILED;
    if (!grad_image && !(grad_T && dL_dfaces_opacity)) return SHADE_DONE;  // nothing arrives, or T's upstream alone, which reaches the opacities alone
    dop = F > 0 ? dL_dfaces_opacity : nullptr;
    dsc = F > 0 ? dL_dface_scale : nullptr;
    dval = grad_image ? dL_dvalues : nullptr;
    return (dop || dsc || dval) ? SHADE_LAUNCH : SHADE_DONE;
}

}  // namespace
}  // namespace dmr
