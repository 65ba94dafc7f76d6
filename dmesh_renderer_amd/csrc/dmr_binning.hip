// dmr_binning.hip -- projection, tile binning and per-tile depth sort (gfx950).
//
// Replaces, for both renderers:
//   preprocessPointCUDA   cuda_rasterizer/forward.cu:17-47   (cuda_renderer/forward.cu:21-52)
//   preprocessFaceCUDA    cuda_rasterizer/forward.cu:76-149  (cuda_renderer/forward.cu:178-260)
//   cub InclusiveSum + duplicateWithKeys + cub SortPairs + identifyTileRanges
//                         cuda_rasterizer/rasterizer_impl.cu:44-124,278-338
//
// The reference emits one (tile<<32 | depth_bits, face) pair per touched tile and runs
// ONE global 64-bit radix sort over all R pairs (k = ceil((32+bit)/8) passes, ~24 B per
// pair per pass).  Here the tile is known at emission time, so pairs are counted and
// scattered straight into their tile's segment (counting sort on the tile digit) and
// each segment is then sorted by (depth_bits, face_id) inside LDS by one workgroup
// (dmr_sort.hpp: the consumer's workgroup of that tile up to 8 192 tiles, k_sort_tiles above).
// Within a (view, tile) a face occurs at most once, so (depth_bits, face_id) is a total
// order and equals the order of the reference's STABLE sort, whose ties keep emission
// order = ascending face id (Q6).  The result -- per-tile face lists and ranges -- is
// bit-identical to the reference's sorted list, whatever order the scatter ran in.
#include <algorithm>
#include <type_traits>

#include "dmr_kernels.hpp"
#include "dmr_sort.hpp"

namespace dmr {

// ---------------------------------------------------------------------------
// 1. per (view, vertex): pixel coordinates, NDC z and the per-view depth attribute packed
//    into one 16-byte record so later stages gather a vertex with a single dwordx4 load.
// ---------------------------------------------------------------------------
// Element k of a [16] column-major matrix whose 4x4 block may be stored transposed (dmr_scene.mats_transposed).
__device__ __forceinline__ float mat_at(const float* __restrict__ m, int k, bool transposed) {
    return m[transposed ? 4 * (k & 3) + (k >> 2) : k];
}

// Also writes the four matrices in contract layout to `mats` ([mv | proj | inv_mv | inv_proj], [B,16] each) in the
// image buffer: every later kernel of the forward and the whole backward read them from there.
__global__ void __launch_bounds__(256)
k_project_verts(int B, int P, const float* __restrict__ verts, const float* __restrict__ mv_mats,
                const float* __restrict__ proj_mats, const float* __restrict__ inv_mv_mats,
                const float* __restrict__ inv_proj_mats, int transposed, const float* __restrict__ verts_depth,
                int W, int H, float4* __restrict__ vproj, float* __restrict__ mats,
                uint32_t* __restrict__ counters, uint32_t ncounters, SegInit seg) {
    {   // every block zeroes a slice of the tile counters (tile_count | tile_hits) the next kernels add into
        const uint32_t per = (ncounters + gridDim.x - 1) / gridDim.x;
        const uint32_t z0 = min(ncounters, blockIdx.x * per), z1 = min(ncounters, z0 + per);
        for (uint32_t i = z0 + threadIdx.x; i < z1; i += 256) counters[i] = 0u;
    }
    if (seg.start) {  // speculative placement (k_bin_faces): segment starts -> offsets and cursors, the order as it stands
        const uint32_t n = seg.ntiles + 1u, per = (n + gridDim.x - 1) / gridDim.x;
        const uint32_t z0 = min(n, blockIdx.x * per), z1 = min(n, z0 + per);
        for (uint32_t i = z0 + threadIdx.x; i < z1; i += 256) {
            const uint32_t o = seg.start[i];
            seg.tile_offset[i] = o;
            if (i < seg.ntiles) { seg.tile_cursor[i] = o; seg.tile_order[i] = seg.order[i]; }
        }
    }
    if (blockIdx.x == 0) {
        for (int i = threadIdx.x; i < 64 * B; i += 256) {
            const int m = i / (16 * B), r = i % (16 * B);
            const float* src = m == 0 ? mv_mats : (m == 1 ? proj_mats : (m == 2 ? inv_mv_mats : inv_proj_mats));
            mats[i] = mat_at(src + 16 * (r >> 4), r & 15, (transposed >> m) & 1);
        }
    }
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)B * P) return;
    const int b = (int)(idx / P), p = (int)(idx % P);
    float mv[16], pr[16];
#pragma unroll
    for (int k = 0; k < 16; k++) {
        mv[k] = mat_at(mv_mats + 16 * b, k, transposed & 1);
        pr[k] = mat_at(proj_mats + 16 * b, k, (transposed >> 1) & 1);
    }
    V3 pv = xform4x3(load_v3(verts, p), mv);
    V4 pc = xform4x4(pv, pr);
    float p_w = (float)(1.0 / (double)clamp_w(pc.w));  // double divide (forward.cu:38)
    V3 n = {pc.x * p_w, pc.y * p_w, pc.z * p_w};
    vproj[idx] = make_float4(ndc2pix(n.x, W), ndc2pix(n.y, H), n.z, verts_depth[idx]);
}

// ---------------------------------------------------------------------------
// 2 / 4. per (view, face): cull, tile rect, sort depth, count the face into every tile of its rect (setup);
//   scatter every (face, tile) pair into its tile's segment, key = depth_bits << 32 | face_id (scatter).
//   rect is kept (packed 4 x u16) so the scatter pass does not redo the float work.
//   Global u32 atomics on ~3000 hot tile counters were the cost of both passes (69 + 80 us at C4 for
//   0.9 M increments; 0.46 + 0.65 ms at C5).  Here a workgroup takes 256 x FPT consecutive faces, counts them
//   into an LDS histogram (ds_add_u32), and touches global memory once per (workgroup, non-empty tile): the count
//   pass adds the bin, the scatter pass reserves the bin's slots with ONE returning atomic and then hands
//   out slots with returning LDS atomics.  The histogram covers a WINDOW of tiles: the bounding box of the
//   workgroup's face rects in the view of its first face (consecutive faces of a mesh are neighbours on screen, so
//   the box is a few hundred tiles even when the image has a million).  Faces with huge rects, faces of another
//   view and whole workgroups whose box exceeds LDS_HIST_MAX tiles use the global counters directly.
// ---------------------------------------------------------------------------
constexpr int LDS_HIST_MAX = 8192;    // 32 KiB of counters
// Faces per thread (FPT): 4 for large meshes -- a long run of consecutive faces per workgroup amortises the window's
// set-up and global atomics -- fewer when that would leave the chip empty: C3's 50 688 faces were 50 workgroups of
// 1024 faces, each thread looping over four 4x4-tile rects (scatter 34 us, 14 us with one face per thread); C4's
// 500 000 faces: set-up / scatter 14.8 / 17.7 us at FPT 4, 13.2 / 14.5 at 2, 14.5 / 16.9 at 1; C5's 8 M: FPT 4.
__host__ inline int bin_fpt(int64_t n) { return n < 256 * 1024 ? 1 : n < 1024 * 1024 ? 2 : 4; }
constexpr uint32_t BIG_RECT = 256;    // tiles; larger rects go straight to global atomics

struct BinWindow { int x0, y0, wx, wy, view; bool lds; };

// Faces whose rect covers more than BIG_RECT tiles (a ground plane, a hull face: up to every tile of the image) are
// not emitted by their own thread -- one thread looping over 8160 tiles with (returning) atomics was 1.9 + 2.2 ms for
// 64 screen-filling triangles at 800x800 (scripts/time_huge.py) -- but queued in LDS and emitted by the whole
// workgroup, 256 tiles at a time.  The queue holds BIG_MAX faces; further ones fall back to their own thread.
constexpr int BIG_MAX = 128;
struct BigFace { uint32_t rect_lo, rect_hi, tile_base, key_lo, key_hi; };

// tiles i = tid, tid + 256, ... of a rect in row-major order, without a division per tile
struct RectWalk {
    uint32_t w, n, i, x, y, dx, dy;
    __device__ __forceinline__ RectWalk(uint32_t minx, uint32_t miny, uint32_t maxx, uint32_t maxy, uint32_t tid) {
        w = maxx - minx; n = w * (maxy - miny); i = tid;
        y = miny + tid / w; x = minx + tid % w; dy = 256u / w; dx = 256u % w;
        x0 = minx;
    }
    uint32_t x0;
    __device__ __forceinline__ bool valid() const { return i < n; }
    __device__ __forceinline__ void next() {
        i += 256u; y += dy; x += dx;
        if (x >= x0 + w) { x -= w; y++; }
    }
};

__device__ __forceinline__ Rect unpack_rect(uint2 r) { return {r.x & 0xffffu, r.x >> 16, r.y & 0xffffu, r.y >> 16}; }

// The LDS of the three face kernels: the window's histogram, its box, the big-face queue.
struct BinShared { uint32_t hist[LDS_HIST_MAX]; int box[4]; BigFace big[BIG_MAX]; uint32_t nbig; };
__device__ __forceinline__ BinShared& bin_shared() { __shared__ BinShared sh; return sh; }

// What a face contributes to the binning: the tiles of its rect (0: culled or off screen), the rect packed 4 x u16, the
// depth its list entries are sorted by (tri: mean z, tet: min z, mapped to [0, 1]) and, tet only, its max depth.
struct FaceBin { uint32_t touched; uint2 rect; float key, max_depth; };
template <bool TET>
__device__ __forceinline__ FaceBin face_bin(int b, int f, int P, const int* __restrict__ faces, const float4* __restrict__ vproj,
                                            int gx, int gy, int r0, int r1) {
    const int v0 = faces[3 * f], v1 = faces[3 * f + 1], v2 = faces[3 * f + 2];
    const float4 a0 = vproj[(int64_t)b * P + v0], a1 = vproj[(int64_t)b * P + v1], a2 = vproj[(int64_t)b * P + v2];
    float max_z = a0.z, min_z = a0.z, depth = 0.0f;
    depth += a0.z;
    max_z = fmaxf(max_z, a1.z); min_z = fminf(min_z, a1.z); depth += a1.z;
    max_z = fmaxf(max_z, a2.z); min_z = fminf(min_z, a2.z); depth += a2.z;
    depth = depth / 3.0f;
    Rect r = {0, 0, 0, 0};
    uint32_t touched = 0u;
    if (!(max_z < -1.0f || min_z > 1.0f)) {
        r = tile_rect({a0.x, a0.y}, {a1.x, a1.y}, {a2.x, a2.y}, gx, gy, r0, r1);
        touched = (r.maxy - r.miny) * (r.maxx - r.minx);
    }
    if (touched == 0) r = {0, 0, 0, 0};
    auto map01 = [](float z) { float d = (z + 1.0f) * 0.5f; if (d < 0.0f) d = 0.0f; if (d > 1.0f) d = 1.0f; return d; };
    return {touched, make_uint2(r.minx | (r.miny << 16), r.maxx | (r.maxy << 16)),
            touched ? (TET ? map01(min_z) : map01(depth)) : 0.0f, TET && touched ? map01(max_z) : 0.0f};
}

// A workgroup's 256 x FPT consecutive (view, face) pairs, FPT per thread; mine: face of the window's view (that of the first one)
template <int FPT>
struct FaceBatch { int64_t base; int view; uint2 rr[FPT]; uint32_t touched[FPT], kd[FPT]; bool mine[FPT]; };
// get(idx, b, f) -> FaceBin, for every pair of the thread
template <int FPT, class Get>
__device__ __forceinline__ FaceBatch<FPT> load_faces(int B, int F, Get get) {
    FaceBatch<FPT> fb;
    fb.base = (int64_t)blockIdx.x * (256 * FPT);
    fb.view = (int)(fb.base / F);
#pragma unroll
    for (int it = 0; it < FPT; it++) {
        const int64_t idx = fb.base + it * 256 + threadIdx.x;
        fb.touched[it] = 0u; fb.rr[it] = make_uint2(0, 0); fb.kd[it] = 0u; fb.mine[it] = false;
        if (idx >= (int64_t)B * F) continue;
        const int b = (int)(idx / F);
        const FaceBin r = get(idx, b, (int)(idx % F));
        fb.touched[it] = r.touched; fb.rr[it] = r.rect; fb.kd[it] = __float_as_uint(r.key); fb.mine[it] = b == fb.view;
    }
    return fb;
}

// Opens the workgroup's window: sh.box = {min x, min y, max x, max y} of the rects that want the LDS histogram, the histogram
// zeroed, the big-face queue empty; uniform result.  Threads reduce their own faces, waves reduce with shuffles, one lane per
// wave touches LDS (every thread doing ds_min / ds_max on the same four words serialises: 2 cycles per lane and atomic).
template <int FPT>
__device__ __forceinline__ BinWindow bin_window(BinShared& sh, const FaceBatch<FPT>& fb) {
    const int tid = threadIdx.x;
    int bx0 = 0x7fffffff, by0 = 0x7fffffff, bx1 = 0, by1 = 0;
#pragma unroll
    for (int it = 0; it < FPT; it++) {
        if (!fb.mine[it] || fb.touched[it] == 0 || fb.touched[it] > BIG_RECT) continue;
        bx0 = min(bx0, (int)(fb.rr[it].x & 0xffffu)); by0 = min(by0, (int)(fb.rr[it].x >> 16));
        bx1 = max(bx1, (int)(fb.rr[it].y & 0xffffu)); by1 = max(by1, (int)(fb.rr[it].y >> 16));
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        bx0 = min(bx0, __shfl_xor(bx0, d, 64)); by0 = min(by0, __shfl_xor(by0, d, 64));
        bx1 = max(bx1, __shfl_xor(bx1, d, 64)); by1 = max(by1, __shfl_xor(by1, d, 64));
    }
    if (tid == 0) { sh.box[0] = 0x7fffffff; sh.box[1] = 0x7fffffff; sh.box[2] = 0; sh.box[3] = 0; sh.nbig = 0u; }
    __syncthreads();
    if ((tid & 63) == 0) {
        atomicMin(&sh.box[0], bx0); atomicMin(&sh.box[1], by0); atomicMax(&sh.box[2], bx1); atomicMax(&sh.box[3], by1);
    }
    __syncthreads();
    BinWindow w;
    w.x0 = sh.box[0]; w.y0 = sh.box[1]; w.wx = sh.box[2] - sh.box[0]; w.wy = sh.box[3] - sh.box[1]; w.view = fb.view;
    w.lds = w.wx > 0 && w.wy > 0 && (int64_t)w.wx * w.wy <= LDS_HIST_MAX;
    if (!w.lds) { w.wx = 0; w.wy = 0; }
    const int nw = w.wx * w.wy;
    for (int t = tid; t < nw; t += 256) sh.hist[t] = 0u;
    __syncthreads();
    return w;
}

// op(bin, its count, tile) for every non-empty bin of the window, a bin per thread
template <class Op>
__device__ __forceinline__ void for_each_bin(BinShared& sh, const BinWindow& w, int gx, int gy, Op op) {
    for (int y = threadIdx.x / 64; y < w.wy; y += 4)
        for (int x = threadIdx.x % 64; x < w.wx; x += 64) {
            const uint32_t c = sh.hist[y * w.wx + x];
            if (c) op(sh.hist[y * w.wx + x], c, (uint32_t)w.view * gx * gy + (uint32_t)(w.y0 + y) * gx + (uint32_t)(w.x0 + x));
        }
}

// Every touched face of the thread: a big one joins the queue with its key (while there is room; the count pass queues the key
// too and ignores it); of any other, for every tile of its rect, in_window(bin, key) or -- no window, another view's face, a
// big face the queue had no room for -- direct(tile, key).
// (Two callables and two loops: one loop over a selected LDS-or-global address compiles to flat atomics.)
template <int FPT, class InWindow, class Direct>
__device__ __forceinline__ void for_each_face_tile(BinShared& sh, const BinWindow& w, const FaceBatch<FPT>& fb, int F, int gx, int gy,
                                                   InWindow in_window, Direct direct) {
#pragma unroll
    for (int it = 0; it < FPT; it++) {
        if (fb.touched[it] == 0) continue;
        const int64_t idx = fb.base + it * 256 + threadIdx.x;
        const uint32_t tb = (uint32_t)(idx / F) * gx * gy;
        const Rect r = unpack_rect(fb.rr[it]);
        const uint64_t key = ((uint64_t)fb.kd[it] << 32) | (uint32_t)(idx % F);
        const bool big = fb.touched[it] > BIG_RECT;
        if (big) {
            const uint32_t q = atomicAdd(&sh.nbig, 1u);
            if (q < (uint32_t)BIG_MAX) { sh.big[q] = BigFace{fb.rr[it].x, fb.rr[it].y, tb, (uint32_t)key, (uint32_t)(key >> 32)}; continue; }
        }
        if (w.lds && fb.mine[it] && !big) {
            for (uint32_t y = r.miny; y < r.maxy; y++)
                for (uint32_t x = r.minx; x < r.maxx; x++) in_window(sh.hist[(y - w.y0) * w.wx + (x - w.x0)], key);
        } else {
            for (uint32_t y = r.miny; y < r.maxy; y++)
                for (uint32_t x = r.minx; x < r.maxx; x++) direct(tb + y * gx + x, key);
        }
    }
}

// op(face, walk) for every queued face, by the whole workgroup (behind a barrier that follows the queueing)
template <class Op>
__device__ __forceinline__ void for_each_big_face(const BinShared& sh, Op op) {
    const uint32_t nbig = min(sh.nbig, (uint32_t)BIG_MAX);
    for (uint32_t q = 0; q < nbig; q++) {
        const BigFace f = sh.big[q];
        const Rect r = unpack_rect(make_uint2(f.rect_lo, f.rect_hi));
        RectWalk t(r.minx, r.miny, r.maxx, r.maxy, threadIdx.x);
        op(f, t);
    }
}

template <bool TET, int FPT>
__global__ void __launch_bounds__(256)
k_setup_faces_lds(int B, int P, int F, const int* __restrict__ faces, const float4* __restrict__ vproj,
                  int gx, int gy, int r0, int r1,
                  uint2* __restrict__ face_rect, float* __restrict__ key_depth, float* __restrict__ max_depth,
                  uint32_t* __restrict__ tiles_touched, uint32_t* __restrict__ tile_count) {
    BinShared& sh = bin_shared();
    const FaceBatch<FPT> fb = load_faces<FPT>(B, F, [&](int64_t idx, int b, int f) {
        const FaceBin r = face_bin<TET>(b, f, P, faces, vproj, gx, gy, r0, r1);
        tiles_touched[idx] = r.touched; face_rect[idx] = r.rect; key_depth[idx] = r.key;
        if (TET) max_depth[idx] = r.max_depth;
        return r;
    });
    const BinWindow w = bin_window(sh, fb);
    // (none of these atomics returns a value)
    for_each_face_tile(sh, w, fb, F, gx, gy, [&](uint32_t& bin, uint64_t) { atomicAdd(&bin, 1u); },
                       [&](uint32_t tile, uint64_t) { atomicAdd(&tile_count[tile], 1u); });
    __syncthreads();
    for_each_bin(sh, w, gx, gy, [&](uint32_t&, uint32_t c, uint32_t tile) { atomicAdd(&tile_count[tile], c); });
    for_each_big_face(sh, [&](const BigFace& f, RectWalk& t) {
        for (; t.valid(); t.next()) atomicAdd(&tile_count[f.tile_base + t.y * gx + t.x], 1u);
    });
}

// ---------------------------------------------------------------------------
// 4, and 2 + 4 in one visit of every face (tri, frames up to SCAN_SINGLE_MAX tiles, a placement exists: dmr_api.hip): ONE
//   emission, bin_emit, with two policies for where a tile's slots end.
//   Exact (k_scatter_faces_lds, SEG = false): the scan laid the segments out from this call's counts, a slot is good below
//   the buffer's capacity, the faces' rects and keys are the set-up pass's.
//   Placed (k_bin_faces, SEG = true): every tile's segment [seg[t], seg[t + 1]) was placed from an earlier call's counts
//   (k_build_placement), the cursors start at the segment starts (k_project_verts), so nothing has to be counted and scanned
//   before entries can be emitted: the workgroup culls / bounds / keys its faces as the set-up pass does (face_bin) and emits.
//   A slot is good below min(seg[t + 1], capacity).  A reservation that ends behind its segment (or behind the buffer) emits
//   NOTHING -- its bin hands out slots from SEG_FULL on, which no buffer holds; the cursor, which advances by the true count all
//   the same, then stands behind the segment's end, which is how the compositing kernels recognise such a tile (they render it
//   empty; the call is redone or flagged) and how the forward's size workgroup (ListSize, dmr_kernels.hpp) sees the overflow;
//   R is the sum of cursor - start.  No workgroup waits for another, and none touches a word that all the others touch.
// ---------------------------------------------------------------------------
constexpr uint32_t SEG_FULL = 0xC0000000u;

// where the entries go; mask_*: where the binning buffer of THIS capacity keeps the coverage masks (dmr_kernels.hpp,
// ImageState::mask_offset), left on the device for the kernels behind (dst null: tet)
struct BinOut { uint32_t* tile_cursor; uint64_t* keys; uint32_t capacity; unsigned long long* mask_offset_dst; unsigned long long mask_offset, mask_first; };

template <int FPT, bool SEG>
__device__ __forceinline__ void bin_emit(const FaceBatch<FPT>& fb, int F, int gx, int gy, const uint32_t* __restrict__ seg, const BinOut& o) {
    if (o.mask_offset_dst && blockIdx.x == 0 && threadIdx.x == 0) { o.mask_offset_dst[0] = o.mask_offset; o.mask_offset_dst[1] = o.mask_first; }
    BinShared& sh = bin_shared();
    auto limit = [&](uint32_t tile) { if constexpr (SEG) return min(seg[tile + 1], o.capacity); else return o.capacity; };
    const BinWindow w = bin_window(sh, fb);
    // pass 1: count this workgroup's entries per tile of the window
#pragma unroll
    for (int it = 0; it < FPT; it++) {
        if (!(w.lds && fb.mine[it]) || fb.touched[it] == 0 || fb.touched[it] > BIG_RECT) continue;
        const Rect r = unpack_rect(fb.rr[it]);
        for (uint32_t y = r.miny; y < r.maxy; y++)
            for (uint32_t x = r.minx; x < r.maxx; x++) atomicAdd(&sh.hist[(y - w.y0) * w.wx + (x - w.x0)], 1u);
    }
    __syncthreads();
    // reserve the workgroup's slots of every non-empty tile with one returning atomic; the bin now holds the cursor
    for_each_bin(sh, w, gx, gy, [&](uint32_t& bin, uint32_t c, uint32_t tile) {
        const uint32_t first = atomicAdd(&o.tile_cursor[tile], c);
        if constexpr (SEG) bin = first + c <= limit(tile) ? first : SEG_FULL;
        else bin = first;
    });
    __syncthreads();
    // pass 2: hand out slots (a bin that did not fit hands out SEG_FULL and up: never below the capacity)
    for_each_face_tile(sh, w, fb, F, gx, gy,
                       [&](uint32_t& bin, uint64_t key) { const uint32_t slot = atomicAdd(&bin, 1u); if (slot < o.capacity) o.keys[slot] = key; },
                       [&](uint32_t tile, uint64_t key) { const uint32_t slot = atomicAdd(&o.tile_cursor[tile], 1u); if (slot < limit(tile)) o.keys[slot] = key; });
    __syncthreads();
    for_each_big_face(sh, [&](const BigFace& f, RectWalk& t) {
        const uint64_t key = ((uint64_t)f.key_hi << 32) | f.key_lo;
        // four returning atomics in flight per thread (one at a time: 0.28 ms for 64 screen-filling faces in one workgroup)
        while (t.valid()) {
            uint32_t tile[4], slot[4], lim[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                tile[u] = 0xffffffffu;
                if (t.valid()) { tile[u] = f.tile_base + t.y * gx + t.x; t.next(); }
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const bool live = tile[u] != 0xffffffffu;
                slot[u] = live ? atomicAdd(&o.tile_cursor[tile[u]], 1u) : 0xffffffffu;
                lim[u] = live ? limit(tile[u]) : 0u;
            }
#pragma unroll
            for (int u = 0; u < 4; u++) if (slot[u] < lim[u]) o.keys[slot[u]] = key;
        }
    });
}

template <int FPT>
__global__ void __launch_bounds__(256)
k_scatter_faces_lds(int B, int F, int gx, int gy, const uint2* __restrict__ face_rect, const float* __restrict__ key_depth,
                    const uint32_t* __restrict__ tiles_touched, BinOut out) {
    const FaceBatch<FPT> fb = load_faces<FPT>(B, F, [&](int64_t idx, int, int) {
        const uint32_t touched = tiles_touched[idx];
        return touched ? FaceBin{touched, face_rect[idx], key_depth[idx], 0.0f} : FaceBin{0u, make_uint2(0, 0), 0.0f, 0.0f};
    });
    bin_emit<FPT, false>(fb, F, gx, gy, nullptr, out);
}

template <int FPT>
__global__ void __launch_bounds__(256)
k_bin_faces(int B, int P, int F, const int* __restrict__ faces, const float4* __restrict__ vproj, int gx, int gy, int r0, int r1,
            float* __restrict__ key_depth, uint32_t* __restrict__ tiles_touched, const uint32_t* __restrict__ seg, BinOut out) {
    const FaceBatch<FPT> fb = load_faces<FPT>(B, F, [&](int64_t idx, int b, int f) {
        const FaceBin r = face_bin<false>(b, f, P, faces, vproj, gx, gy, r0, r1);
        tiles_touched[idx] = r.touched; key_depth[idx] = r.key;
        return r;
    });
    bin_emit<FPT, true>(fb, F, gx, gy, seg, out);
}

// ---------------------------------------------------------------------------
// 3. exclusive scan of the per-tile counts -> segment starts (= the reference's `ranges`),
//    cursor copy for the scatter, and R.  One workgroup: n = B * tiles is small (C4: 8160).
// ---------------------------------------------------------------------------
// Also emits tile_order: the tiles bucket-sorted by descending list length (64 buckets of 16 entries).  The
// compositing kernels take their tile from it, longest first: with C4's lengths (64..650 entries, busy tiles
// clustered) dispatch in image order finishes 33 % above the ideal makespan, longest-first 10 % (simulated on the
// measured length distribution).
constexpr int ORDER_BUCKETS = 64;
__device__ __forceinline__ int order_bucket(uint32_t n) { return ORDER_BUCKETS - 1 - (int)min(n >> 4, (uint32_t)(ORDER_BUCKETS - 1)); }
// Neighbouring tiles have lists of similar length, so the lanes of a wave mostly want the SAME bucket, and same-address
// LDS atomics retire one lane at a time (scripts/micro/lds_atomics.hip).  Every bucket therefore has ORDER_COPIES
// counters, picked by lane: at most four lanes of a wave meet on one.  The order inside a bucket is arbitrary anyway.
// (Measured: on its own this changed nothing at C4 -- 16.4 us before and after; the kernel's time was its uncoalesced
// global accesses, see the slab below.  Kept: it bounds the worst case of a frame whose busy tiles share one bucket.)
constexpr int ORDER_COPIES = 16;
constexpr int ORDER_CELLS = ORDER_BUCKETS * ORDER_COPIES;  // + 1 cell for the empty tiles, behind all the others
__device__ __forceinline__ int order_cell(uint32_t n, int lane) { return order_bucket(n) * ORDER_COPIES + (lane & (ORDER_COPIES - 1)); }

// Both scans are one 1024-thread workgroup up to SCAN_SLAB tiles (C4: 8160), SCAN_BATCH tiles per thread.
constexpr int SCAN_BATCH = 8;

__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t local, int tid, uint32_t* wave_sum /*[17]*/) {
    const int lane = tid & 63, wave = tid >> 6;
    uint32_t incl = local;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        uint32_t o = __shfl_up(incl, d, 64);
        if (lane >= d) incl += o;
    }
    if (lane == 63) wave_sum[wave] = incl;
    __syncthreads();
    if (tid < 64) {
        const uint32_t w = tid < 16 ? wave_sum[tid] : 0u;
        uint32_t wi = w;
#pragma unroll
        for (int d = 1; d < 16; d <<= 1) {
            uint32_t o = __shfl_up(wi, d, 64);
            if (tid >= d) wi += o;
        }
        if (tid < 16) wave_sum[tid] = wi - w;
        if (tid == 15) wave_sum[16] = wi;
    }
    __syncthreads();
    return wave_sum[wave] + incl - local;  // total in wave_sum[16]
}

// One workgroup has one memory pipeline: a thread touching its 8 consecutive tiles directly (32-byte stride across a
// wave) made every lane a request of its own -- 24 stores + 16 loads per thread, 11 of the kernel's 17 us in the
// store pass alone.  So the tiles go through an LDS slab: coalesced global loads in, 16-byte LDS reads per thread, and
// offsets / order are written back to the slab and leave as coalesced stores.
constexpr int SCAN_SLAB = 1024 * SCAN_BATCH;  // tiles one workgroup scans (LDS: 32 KB)

__device__ __forceinline__ void slab_load(uint32_t* __restrict__ slab, const uint32_t* __restrict__ src, int n, int tid) {
#pragma unroll
    for (int j = 0; j < SCAN_BATCH; j++) { const int i = j * 1024 + tid; slab[i] = i < n ? src[i] : 0u; }
}
__device__ __forceinline__ void slab_read(const uint32_t* __restrict__ slab, int tid, uint32_t (&c)[SCAN_BATCH]) {
    static_assert(SCAN_BATCH == 8, "two 16-byte LDS reads per thread");
    const uint4 lo = *reinterpret_cast<const uint4*>(slab + tid * SCAN_BATCH), hi = *reinterpret_cast<const uint4*>(slab + tid * SCAN_BATCH + 4);
    c[0] = lo.x; c[1] = lo.y; c[2] = lo.z; c[3] = lo.w; c[4] = hi.x; c[5] = hi.y; c[6] = hi.z; c[7] = hi.w;
}
// the thread's exclusive running offsets, starting at `run`, over its own slots of the slab
__device__ __forceinline__ void slab_write_offsets(uint32_t* __restrict__ slab, int tid, uint32_t run, const uint32_t (&c)[SCAN_BATCH]) {
    uint32_t o[SCAN_BATCH];
#pragma unroll
    for (int j = 0; j < SCAN_BATCH; j++) { o[j] = run; run += c[j]; }
    *reinterpret_cast<uint4*>(slab + tid * SCAN_BATCH) = make_uint4(o[0], o[1], o[2], o[3]);
    *reinterpret_cast<uint4*>(slab + tid * SCAN_BATCH + 4) = make_uint4(o[4], o[5], o[6], o[7]);
}

__global__ void __launch_bounds__(1024)
k_scan_tiles(int n, const uint32_t* __restrict__ tile_count, uint32_t* __restrict__ tile_offset,
             uint32_t* __restrict__ tile_cursor, int* __restrict__ num_rendered, uint32_t* __restrict__ tile_order, SizeOut out) {
    static_assert(ORDER_CELLS == 1024, "one counter cell per thread");
    __shared__ uint32_t wave_sum[17];
    __shared__ uint32_t bucket[ORDER_CELLS + 1];
    __shared__ __attribute__((aligned(16))) uint32_t slab[SCAN_SLAB];
    const int tid = threadIdx.x, lane = tid & 63;
    const int begin = tid * SCAN_BATCH;  // n <= SCAN_SLAB
    bucket[tid] = 0u;
    slab_load(slab, tile_count, n, tid);
    __syncthreads();
    uint32_t c[SCAN_BATCH], local = 0;
    slab_read(slab, tid, c);
#pragma unroll
    for (int j = 0; j < SCAN_BATCH; j++) {
        local += c[j];
        if (c[j]) atomicAdd(&bucket[order_cell(c[j], lane)], 1u);  // empty tiles: what is left over
    }
    const uint32_t run = block_exclusive_scan(local, tid, wave_sum);
    const uint32_t total = wave_sum[16];
    slab_write_offsets(slab, tid, run, c);
    __syncthreads();  // wave_sum is reused; the offsets are in the slab
    // exclusive scan of the cells (bucket-major): bucket 0 holds the longest lists, empty tiles come last
    const uint32_t cell_base = block_exclusive_scan(bucket[tid], tid, wave_sum);
    bucket[tid] = cell_base;
    if (tid == 0) bucket[ORDER_CELLS] = wave_sum[16];
#pragma unroll
    for (int j = 0; j < SCAN_BATCH; j++) {
        const int i = j * 1024 + tid;
        if (i < n) { const uint32_t o = slab[i]; tile_offset[i] = o; tile_cursor[i] = o; }
    }
    __syncthreads();  // the cells are final; the slab is free
#pragma unroll
    for (int j = 0; j < SCAN_BATCH; j++) {
        const bool in = begin + j < n;
        const bool empty = in && c[j] == 0u;
        const uint64_t em = __ballot(empty);  // empty tiles (most of a frame) share one cell: claimed per wave
        uint32_t ebase = 0;
        if (em) {
            const int leader = __ffsll((long long)em) - 1;
            if (lane == leader) ebase = atomicAdd(&bucket[ORDER_CELLS], (uint32_t)__popcll(em));
            ebase = __shfl(ebase, leader, 64);
        }
        if (empty) slab[ebase + (uint32_t)__popcll(em & ((1ull << lane) - 1ull))] = (uint32_t)(begin + j);
        else if (in) slab[atomicAdd(&bucket[order_cell(c[j], lane)], 1u)] = (uint32_t)(begin + j);
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < SCAN_BATCH; j++) { const int i = j * 1024 + tid; if (i < n) tile_order[i] = slab[i]; }
    if (tid == 0) {
        tile_offset[n] = total; *num_rendered = (int)total;
        out.publish(total);
    }
}

// The placement k_bin_faces speculates on, built from the exact counts of a call that went through set-up -> scan ->
// scatter: tile t gets room for its count + 25 % + SEG_SLACK entries (so that a tile that was empty can receive a few),
// segments in tile order, start[n] = the padded total; the order is that call's (longest list first), which
// build_placement (dmr_api.hip) then replaces by the XCD-local one of dmr_tile_order.hpp -- every tile has a segment, so
// every tile's position is a first-chunk mask slot whatever the order.  One workgroup, n <= SCAN_SLAB.
__global__ void __launch_bounds__(1024)
k_build_placement(int n, const uint32_t* __restrict__ tile_count, const uint32_t* __restrict__ tile_order,
                  uint32_t* __restrict__ start, uint32_t* __restrict__ order) {
    __shared__ uint32_t wave_sum[17];
    __shared__ __attribute__((aligned(16))) uint32_t slab[SCAN_SLAB];
    const int tid = threadIdx.x;
    slab_load(slab, tile_count, n, tid);
    __syncthreads();
    uint32_t c[SCAN_BATCH], local = 0;
    slab_read(slab, tid, c);
#pragma unroll
    for (int j = 0; j < SCAN_BATCH; j++) {
        c[j] = tid * SCAN_BATCH + j < n ? c[j] + (c[j] >> 2) + SEG_SLACK : 0u;
        local += c[j];
    }
    const uint32_t run = block_exclusive_scan(local, tid, wave_sum);
    slab_write_offsets(slab, tid, run, c);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < SCAN_BATCH; j++) {
        const int i = j * 1024 + tid;
        if (i < n) { start[i] = slab[i]; order[i] = tile_order[i]; }
    }
    if (tid == 0) start[n] = wave_sum[16];
}

// Records a tile's region of the backward's record buffer must hold.  The per-pixel kernel writes a face's blended pairs
// as one run padded to a multiple of HIT_GROUP records (the hit-parallel kernel takes HIT_GROUP records of ONE list entry
// per lane), so a tile with h blended pairs (counted by the forward) in a list of `len` entries needs at most
// h + (HIT_GROUP - 1) * min(len, h) records; rounded up to whole blocks of HIT_BLOCK records (the layout inside a region,
// dmr_kernels.hpp).
// (record_bound: dmr_kernels.hpp)

// ---- the same for many tiles (B * tiles > SCAN_SINGLE_MAX: several views at 1080p, 4096^2 images): one workgroup
// per 8192 tiles, three small launches (partial sums + bucket sizes | scan of the partials | offsets + order) instead
// of one workgroup streaming everything (0.5 ms for C5's 1 M tiles).
constexpr int SCAN_BLOCK_TILES = 8192;
static_assert(SCAN_SINGLE_MAX == SCAN_SLAB, "up to here one workgroup does it all (k_scan_tiles, k_scan_hits)");

// pass 1: blk_sum[block] = sum of the block's counts; bucket_count[b] += tiles of the block in order bucket b
// (ORDER == false: the scan of the backward's record regions; the counts are record_bound(tile_count, list length))
template <bool ORDER>
__global__ void __launch_bounds__(1024)
k_scan_tiles_partial(int n, const uint32_t* __restrict__ tile_count, const uint32_t* __restrict__ len_offset, uint32_t* __restrict__ blk_sum,
                     uint32_t* __restrict__ bucket_count) {
    __shared__ uint32_t wave_sum[17];
    __shared__ uint32_t bucket[ORDER_CELLS];
    const int tid = threadIdx.x, lane = tid & 63;
    const int begin = min(n, (int)blockIdx.x * SCAN_BLOCK_TILES + tid * SCAN_BATCH), end = min(n, begin + SCAN_BATCH);
    if (ORDER) bucket[tid] = 0u;
    __syncthreads();
    uint32_t c[SCAN_BATCH], local = 0;
#pragma unroll
    for (int j = 0; j < SCAN_BATCH; j++) {
        c[j] = begin + j < end ? tile_count[begin + j] : 0u;
        if (!ORDER && begin + j < end) c[j] = record_bound(c[j], len_offset[begin + j + 1] - len_offset[begin + j]);
    }
#pragma unroll
    for (int j = 0; j < SCAN_BATCH; j++) {
        local += c[j];
        if (ORDER && begin + j < end && c[j]) atomicAdd(&bucket[order_cell(c[j], lane)], 1u);
    }
    block_exclusive_scan(local, tid, wave_sum);  // (its barriers also publish the cells)
    if (tid == 0) blk_sum[blockIdx.x] = wave_sum[16];
    if (ORDER && tid < ORDER_BUCKETS) {
        uint32_t cnt = 0;
#pragma unroll
        for (int q = 0; q < ORDER_COPIES; q++) cnt += bucket[tid * ORDER_COPIES + q];
        if (cnt) atomicAdd(&bucket_count[tid], cnt);
    }
}

// pass 2 (one workgroup): blk_sum -> exclusive scan in place, total -> R; bucket_count -> exclusive scan in place
// (bucket 0 = longest lists first, empty tiles last): the cursors pass 3 claims from
__global__ void __launch_bounds__(1024)
k_scan_tiles_blocks(int nblk, int n, uint32_t* __restrict__ blk_sum, uint32_t* __restrict__ bucket_count,
                    uint32_t* __restrict__ tile_offset, int* __restrict__ num_rendered, unsigned long long* __restrict__ total64, SizeOut out) {
    __shared__ uint32_t wave_sum[17];
    const int tid = threadIdx.x, lane = tid & 63;
    unsigned long long carry = 0;  // the 32-bit offsets wrap harmlessly when the total does not fit (the host checks it)
    for (int i0 = 0; i0 < nblk; i0 += 1024) {
        const uint32_t v = i0 + tid < nblk ? blk_sum[i0 + tid] : 0u;
        const uint32_t ex = block_exclusive_scan(v, tid, wave_sum);
        if (i0 + tid < nblk) blk_sum[i0 + tid] = (uint32_t)carry + ex;
        carry += wave_sum[16];
        __syncthreads();  // wave_sum is reused
    }
    if (tid == 0) {
        tile_offset[n] = (uint32_t)carry;
        if (num_rendered) *num_rendered = (int)carry;  // (one of the two device totals: the forward's R, the backward's records)
        if (total64) *total64 = carry;
        out.publish(carry);
    }
    if (bucket_count && tid < 128) {  // waves 0 and 1; only wave 0 holds buckets 0..63, the empty-tile bucket follows them
        const uint32_t c = tid < ORDER_BUCKETS ? bucket_count[tid] : 0u;
        uint32_t bi = c;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            uint32_t o = __shfl_up(bi, d, 64);
            if (lane >= d) bi += o;
        }
        if (tid < ORDER_BUCKETS) bucket_count[tid] = bi - c;
        if (tid == ORDER_BUCKETS - 1) bucket_count[ORDER_BUCKETS] = bi;
    }
}

// pass 3: offsets, cursors and the order
template <bool ORDER>
__global__ void __launch_bounds__(1024)
k_scan_tiles_final(int n, const uint32_t* __restrict__ tile_count, const uint32_t* __restrict__ len_offset, const uint32_t* __restrict__ blk_sum,
                   uint32_t* __restrict__ bucket_cursor, uint32_t* __restrict__ tile_offset, uint32_t* __restrict__ tile_cursor,
                   uint32_t* __restrict__ tile_order) {
    __shared__ uint32_t wave_sum[17];
    __shared__ uint32_t bucket[ORDER_CELLS + 1];
    const int tid = threadIdx.x, lane = tid & 63;
    const int begin = min(n, (int)blockIdx.x * SCAN_BLOCK_TILES + tid * SCAN_BATCH), end = min(n, begin + SCAN_BATCH);
    if (ORDER) { bucket[tid] = 0u; if (tid == 0) bucket[ORDER_CELLS] = 0u; }
    __syncthreads();
    uint32_t c[SCAN_BATCH], local = 0;
    int n_empty = 0;
#pragma unroll
    for (int j = 0; j < SCAN_BATCH; j++) {
        c[j] = begin + j < end ? tile_count[begin + j] : 0u;
        if (!ORDER && begin + j < end) {  // record regions: the bound, and tile_used (here: tile_cursor) cleared
            c[j] = record_bound(c[j], len_offset[begin + j + 1] - len_offset[begin + j]);
            tile_cursor[begin + j] = 0u;
        }
    }
#pragma unroll
    for (int j = 0; j < SCAN_BATCH; j++) {
        local += c[j];
        if (ORDER && begin + j < end) {
            if (c[j]) atomicAdd(&bucket[order_cell(c[j], lane)], 1u);
            else n_empty++;
        }
    }
    if (ORDER) {  // empty tiles of the block: one LDS add per wave
        n_empty = wave_total(n_empty);
        if (lane == 0 && n_empty) atomicAdd(&bucket[ORDER_CELLS], (uint32_t)n_empty);
    }
    uint32_t run = blk_sum[blockIdx.x] + block_exclusive_scan(local, tid, wave_sum);
    // claim the block's share of every bucket of the global order; the LDS cells then hand out slots
    if (ORDER && tid < ORDER_BUCKETS) {
        uint32_t cnt = 0;
#pragma unroll
        for (int q = 0; q < ORDER_COPIES; q++) cnt += bucket[tid * ORDER_COPIES + q];
        uint32_t base = cnt ? atomicAdd(&bucket_cursor[tid], cnt) : 0u;
#pragma unroll
        for (int q = 0; q < ORDER_COPIES; q++) { const uint32_t k = bucket[tid * ORDER_COPIES + q]; bucket[tid * ORDER_COPIES + q] = base; base += k; }
    }
    if (ORDER && tid == ORDER_BUCKETS) { const uint32_t cnt = bucket[ORDER_CELLS]; bucket[ORDER_CELLS] = cnt ? atomicAdd(&bucket_cursor[ORDER_BUCKETS], cnt) : 0u; }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < SCAN_BATCH; j++) {
        const bool in = begin + j < end;
        if (in) { tile_offset[begin + j] = run; if (ORDER) tile_cursor[begin + j] = run; }
        run += c[j];
        if (!ORDER) continue;
        const bool empty = in && c[j] == 0u;
        const uint64_t em = __ballot(empty);
        uint32_t ebase = 0;
        if (em) {
            const int leader = __ffsll((long long)em) - 1;
            if (lane == leader) ebase = atomicAdd(&bucket[ORDER_CELLS], (uint32_t)__popcll(em));
            ebase = __shfl(ebase, leader, 64);
        }
        if (empty) tile_order[ebase + (uint32_t)__popcll(em & ((1ull << lane) - 1ull))] = (uint32_t)(begin + j);
        else if (in) tile_order[atomicAdd(&bucket[order_cell(c[j], lane)], 1u)] = (uint32_t)(begin + j);
    }
}

// exclusive scan of those bounds: every tile's region of the backward's record buffer (u32 offsets; the total is < 2^32 or
// the backward fails) and the total.  Also clears tile_used (records the per-pixel kernel really wrote, per tile).
__global__ void __launch_bounds__(1024)
k_scan_hits(int n, const uint32_t* __restrict__ tile_hits, const uint32_t* __restrict__ tile_offset, const uint32_t* __restrict__ tile_end,
            uint32_t* __restrict__ hit_offset,
            uint32_t* __restrict__ tile_used, unsigned long long* __restrict__ hit_total, SizeOut out) {
    __shared__ uint32_t wave_sum[17];
    __shared__ unsigned long long s_total;
    __shared__ __attribute__((aligned(16))) uint32_t slab[SCAN_SLAB];
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid == 0) s_total = 0ull;
#pragma unroll
    for (int j = 0; j < SCAN_BATCH; j++) {  // n <= SCAN_SLAB
        const int i = j * 1024 + tid;
        slab[i] = i < n ? record_bound(tile_hits[i], list_end(tile_offset, tile_end, i) - tile_offset[i]) : 0u;
        if (i < n) tile_used[i] = 0u;
    }
    __syncthreads();
    uint32_t c[SCAN_BATCH], local = 0;
    slab_read(slab, tid, c);
    unsigned long long wide = 0;
#pragma unroll
    for (int j = 0; j < SCAN_BATCH; j++) { local += c[j]; wide += c[j]; }
    // 64-bit total (overflow check on the host); the offsets themselves wrap harmlessly in that case
    wide = wave_total(wide);
    const uint32_t run = block_exclusive_scan(local, tid, wave_sum);
    if (lane == 0) atomicAdd(&s_total, wide);
    slab_write_offsets(slab, tid, run, c);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < SCAN_BATCH; j++) { const int i = j * 1024 + tid; if (i < n) hit_offset[i] = slab[i]; }
    if (tid == 0) {
        hit_offset[n] = wave_sum[16]; *hit_total = s_total;
        out.publish(s_total);
    }
}

// ---------------------------------------------------------------------------
// 5. per-tile sort by (depth_bits, face_id) as a kernel of its own (the tet path; the tri forward sorts its tile itself):
//    dmr_sort.hpp.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_sort_tiles(uint32_t ntiles, const uint32_t* __restrict__ tile_offset, const uint32_t* __restrict__ tile_order,
             uint64_t* __restrict__ keys, uint32_t* __restrict__ face_list, uint32_t capacity) {
    __shared__ uint64_t s_keys[SORT_LDS_KEYS];
    __shared__ uint32_t s_rank[SORT_LDS_KEYS];
    // grid-stride over tiles: most tiles of a frame are empty, a workgroup launch per tile costs more than the sort
    for (uint32_t ti = blockIdx.x; ti < ntiles; ti += gridDim.x) {
        const uint32_t tile = tile_order[ti];  // longest first
        const uint32_t begin = tile_offset[tile], end = tile_offset[tile + 1];
        // (a list beyond the buffer exists only while a size guess is being refuted: everything is redone then)
        if (end == begin || end > capacity) continue;
        __syncthreads();  // the previous tile's keys are no longer needed
        sort_tile(begin, end - begin, keys, face_list, s_keys, s_rank, threadIdx.x);
    }
}

// ---------------------------------------------------------------------------
// host launchers
// ---------------------------------------------------------------------------
void launch_project_verts(const dmr_scene& s, const Dims& d, const Scratch& c, SegInit seg, hipStream_t st) {
    const ImageState& is = c.is;
    const int64_t n = (int64_t)s.B * s.P;
    if (seg.start) { seg.tile_offset = is.tile_offset; seg.tile_cursor = is.tile_cursor; seg.tile_order = is.tile_order; seg.ntiles = (uint32_t)d.ntiles; }
    StageScope t(DMR_STAGE_PROJECT, st);
    k_project_verts<<<dim3((unsigned)std::max<int64_t>(1, (n + 255) / 256)), dim3(256), 0, st>>>(
        s.B, s.P, s.verts, s.mv_mats, s.proj_mats, s.inv_mv_mats, s.inv_proj_mats, s.mats_transposed, s.verts_depth,
        s.W, s.H, c.ps.vproj, is.mats, is.tile_count, (uint32_t)(is.scan_tmp + SCAN_TMP_BUCKETS - is.tile_count), seg);
}

// fn(std::integral_constant<int, FPT>, grid): the faces per thread of n (view, face) pairs and their workgroups
template <class Fn>
void with_fpt(int64_t n, Fn fn) {
    const int fpt = bin_fpt(n);
    const dim3 grid((unsigned)std::max<int64_t>(1, (n + 256 * fpt - 1) / (256 * fpt)));
    if (fpt == 1) fn(std::integral_constant<int, 1>{}, grid);
    else if (fpt == 2) fn(std::integral_constant<int, 2>{}, grid);
    else fn(std::integral_constant<int, 4>{}, grid);
}

void launch_setup_faces(const dmr_scene& s, const Dims& d, const Scratch& c, bool tet, hipStream_t st) {
    const FaceState& fs = c.fs;
    const int64_t n = (int64_t)s.B * s.F;
    if (n == 0) return;
    StageScope t(DMR_STAGE_SETUP_FACES, st);
    with_fpt(n, [&](auto fpt, dim3 grid) {
        auto k = tet ? k_setup_faces_lds<true, fpt()> : k_setup_faces_lds<false, fpt()>;
        k<<<grid, dim3(256), 0, st>>>(s.B, s.P, s.F, s.faces, c.ps.vproj, d.gx, d.gy, d.r0, d.r1, fs.rect, fs.key_depth, fs.max_depth,
                                      fs.tiles_touched, c.is.tile_count);
    });
}

void launch_scan_tiles(const Dims& d, const Scratch& c, SizeOut out, hipStream_t st) {
    const ImageState& is = c.is;
    const int ntiles = d.ntiles;
    StageScope t(DMR_STAGE_SCAN, st);
    if (ntiles <= SCAN_SINGLE_MAX) {
        k_scan_tiles<<<dim3(1), dim3(1024), 0, st>>>(ntiles, is.tile_count, is.tile_offset, is.tile_cursor, is.num_rendered, is.tile_order, out);
        return;
    }
    // scan_tmp: [ORDER_BUCKETS + 1 bucket counters, zeroed by k_project_verts | partial sums per block]
    const int nblk = (ntiles + SCAN_BLOCK_TILES - 1) / SCAN_BLOCK_TILES;
    uint32_t* bucket = is.scan_tmp;
    uint32_t* blk_sum = is.scan_tmp + SCAN_TMP_BUCKETS;
    k_scan_tiles_partial<true><<<dim3(nblk), dim3(1024), 0, st>>>(ntiles, is.tile_count, nullptr, blk_sum, bucket);
    k_scan_tiles_blocks<<<dim3(1), dim3(1024), 0, st>>>(nblk, ntiles, blk_sum, bucket, is.tile_offset, is.num_rendered, nullptr, out);
    k_scan_tiles_final<true><<<dim3(nblk), dim3(1024), 0, st>>>(ntiles, is.tile_count, nullptr, blk_sum, bucket, is.tile_offset, is.tile_cursor, is.tile_order);
}

size_t scan_tmp_words(int ntiles) { return SCAN_TMP_BUCKETS + (size_t)(ntiles + SCAN_BLOCK_TILES - 1) / SCAN_BLOCK_TILES + 1; }

void launch_scan_hits(const Dims& d, const Scratch& c, SizeOut out, hipStream_t st) {
    const ImageState& is = c.is;
    const int ntiles = d.ntiles;
    StageScope t(DMR_STAGE_SCAN, st);
    if (ntiles <= SCAN_SINGLE_MAX) {
        k_scan_hits<<<dim3(1), dim3(1024), 0, st>>>(ntiles, is.tile_hits, is.tile_offset, is.tile_cursor, is.hit_offset, is.tile_used, is.hit_total, out);
        return;
    }
    const int nblk = (ntiles + SCAN_BLOCK_TILES - 1) / SCAN_BLOCK_TILES;
    uint32_t* blk_sum = is.scan_tmp + SCAN_TMP_BUCKETS;  // the forward's partial sums are no longer needed
    k_scan_tiles_partial<false><<<dim3(nblk), dim3(1024), 0, st>>>(ntiles, is.tile_hits, is.tile_offset, blk_sum, nullptr);
    k_scan_tiles_blocks<<<dim3(1), dim3(1024), 0, st>>>(nblk, ntiles, blk_sum, nullptr, is.hit_offset, nullptr, is.hit_total, out);
    k_scan_tiles_final<false><<<dim3(nblk), dim3(1024), 0, st>>>(ntiles, is.tile_hits, is.tile_offset, blk_sum, nullptr, is.hit_offset, is.tile_used, nullptr);
}

// where the emit pass of either binning policy writes: the cursors, the binning buffer's keys, the masks' place
static BinOut bin_out(const Scratch& c, bool masks) {
    return BinOut{c.is.tile_cursor, c.bs.keys, c.bs.capacity, masks ? c.is.mask_offset : nullptr, c.bs.mask_offset, c.bs.mask_first};
}

void launch_scatter_faces(const dmr_scene& s, const Dims& d, const Scratch& c, bool masks, hipStream_t st) {
    const int64_t n = (int64_t)s.B * s.F;
    if (n == 0) return;
    StageScope t(DMR_STAGE_SCATTER, st);
    const BinOut out = bin_out(c, masks);
    with_fpt(n, [&](auto fpt, dim3 grid) {
        k_scatter_faces_lds<fpt()><<<grid, dim3(256), 0, st>>>(s.B, s.F, d.gx, d.gy, c.fs.rect, c.fs.key_depth, c.fs.tiles_touched, out);
    });
}

void launch_bin_faces(const dmr_scene& s, const Dims& d, const Scratch& c, hipStream_t st) {
    StageScope t(DMR_STAGE_SCATTER, st);
    const BinOut out = bin_out(c, true);
    with_fpt((int64_t)s.B * s.F, [&](auto fpt, dim3 grid) {
        k_bin_faces<fpt()><<<grid, dim3(256), 0, st>>>(s.B, s.P, s.F, s.faces, c.ps.vproj, d.gx, d.gy, d.r0, d.r1, c.fs.key_depth,
                                                      c.fs.tiles_touched, c.is.tile_offset, out);
    });
}

void launch_build_placement(int ntiles, const uint32_t* tile_count, const uint32_t* tile_order, uint32_t* start, uint32_t* order,
                            hipStream_t st) {
    StageScope t(DMR_STAGE_SCAN, st);
    k_build_placement<<<dim3(1), dim3(1024), 0, st>>>(ntiles, tile_count, tile_order, start, order);
}

void launch_sort_tiles(const Dims& d, const Scratch& c, hipStream_t st) {
    if (d.ntiles == 0) return;
    StageScope t(DMR_STAGE_SORT, st);
    k_sort_tiles<<<dim3((unsigned)std::min(d.ntiles, 256 * 64)), dim3(256), 0, st>>>((uint32_t)d.ntiles, c.is.tile_offset, c.is.tile_order, c.bs.keys,
                                                                                    c.bs.face_list, c.bs.capacity);
}

}  // namespace dmr
