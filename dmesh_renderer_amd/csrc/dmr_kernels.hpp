// dmr_kernels.hpp -- internal launcher declarations (host side of the gfx950 kernels).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdlib>
#include <type_traits>

#include "../../include/dmesh_renderer_amd.h"
#include "dmr_device.hpp"

namespace dmr {

// Packed gradient accumulators of the backward passes (DMR_BUF_WORK):
//   vertex row  [B][P][8] = { dx, dy, dz, dr, dg, db, ddepth, - }   one 32-byte row per (view, vertex)
//   face row    [B][F][2] = { dopacity, dintense }
// so that one (tile, face) flush touches 3 vertex rows + 1 face row (4 memory-side atomic
// requests) instead of 23 scattered dwords.
constexpr int VROW = 8;
constexpr int FROW = 2;
// Records of one list entry (one face in one tile) form a run padded to a multiple of HIT_GROUP; the hit-parallel backward
// takes one group per lane (k_tri_backward_pix / k_tri_backward_hits, dmr_tri.hip).
constexpr int HIT_GROUP = 4;
// Inside a tile's region the records are stored in blocks of HIT_BLOCK = 64 groups, record q of group l of a block at
// block * HIT_BLOCK + q * 64 + l: the 64 lanes of a wave read record q of their groups as one contiguous kilobyte
// (16 cache lines; 64 bytes per lane in memory order would be 64 lines per load instruction, and the hit-parallel kernel
// is bound by exactly that: line accesses in the texture addresser).  Regions are whole blocks.
constexpr int HIT_BLOCK = 64 * HIT_GROUP;
__host__ __device__ inline uint32_t hit_slot_address(uint32_t rel) {  // rel: record index in the tile's face-major order
    return (rel & ~(uint32_t)(HIT_BLOCK - 1)) + (rel & (uint32_t)(HIT_GROUP - 1)) * 64u + ((rel & (uint32_t)(HIT_BLOCK - 1)) / (uint32_t)HIT_GROUP);
}

// Record region of a tile: a face's records form one run padded to a multiple of HIT_GROUP, so a tile with h blended pairs
// (counted by the forward) in a list of `len` entries needs at most h + (HIT_GROUP - 1) * min(len, h) records, rounded up to
// whole blocks.
__host__ __device__ inline uint32_t record_bound(uint32_t h, uint32_t len) {
    if (h == 0u) return 0u;
    const uint32_t b = h + (uint32_t)(HIT_GROUP - 1) * (len < h ? len : h);
    return (b + (uint32_t)(HIT_BLOCK - 1)) & ~(uint32_t)(HIT_BLOCK - 1);
}
// Up to this many tiles one workgroup scans them all (k_scan_tiles, k_scan_hits), and k_tri_backward_pix can find its tile's
// record region on its own (HitRegions below).
constexpr int SCAN_SINGLE_MAX = 8192;

// fn(std::bool_constant<b>{}): a run-time flag picks the compile-time variant of a kernel (ALPHA, SORT, ...)
template <class Fn>
void with_flag(bool b, Fn fn) {
    if (b) fn(std::true_type{});
    else fn(std::false_type{});
}
#ifdef DMR_ABLATION
// the DMR_ABLATE bits the kernels' parameter blocks carry (ablation build only)
inline int ablate_bits() { static const int dbg = getenv("DMR_ABLATE") ? atoi(getenv("DMR_ABLATE")) : 0; return dbg; }
#endif

// ---- per-stage HIP-event timing (dmr_api.hip); a no-op unless dmr_profile_enable() set the stage's bit
struct StageScope {
    int stage; hipStream_t st; void* rec;
    StageScope(int stage, hipStream_t st);
    ~StageScope();
};

// ---- a call's scratch: the four buffers' views, carved by dmr_api.hip (carve_*), read by every launcher's make_params
struct Dims { int gx, gy, r0, r1, ntiles; size_t BP, BF, npix; };
struct TetSeq;
struct PointState { float4* vproj; };
struct FaceState {
    uint2* rect; float* key_depth; float* max_depth; uint32_t* tiles_touched;
    void* facerec; void* colrec; void* tetrec;  // tet: packed march records (dmr_tet.hip)
};
// (tile_count and FaceState::rect belong to the exact policy of the binning: the set-up pass leaves them for the scan and the
// scatter.  Behind launch_bin_faces tile_count stays zero -- a tile's count is tile_cursor - tile_offset there -- and rect keeps
// what an earlier call left; nothing reads either afterwards)
struct ImageState {
    uint32_t* tile_count; uint32_t* tile_offset; int* num_rendered;
    uint32_t* tile_cursor;  // every tile's list end (list_end() below): the cursors the entries were emitted through
    float* final_T; float* final_prev_T; uint32_t* n_contrib;  // (tet: the logarithms of T)
    uint32_t* tile_hits;    // tri: covered (pixel, face) pairs below n_contrib per tile, counted by the forward
    uint32_t* tile_bound;   // record_bound(tile_hits, list length), written next to it (16-byte aligned, zero for empty tiles)
    uint32_t* scan_tmp;
    uint32_t* hit_offset;   // record regions: exclusive scan of the tiles' record bounds (k_scan_hits, backward)
    uint32_t* tile_used;    // records k_tri_backward_pix wrote into a tile's region (padded runs; <= the bound)
    unsigned long long* hit_total;
    uint32_t* tile_order;   // all B * gx * gy tiles, longest list first (k_scan_tiles)
    int32_t* first_face; int32_t* first_tet; int32_t* last_face; int32_t* last_tet; uint8_t* is_active;
    float* mats;  // [mv | proj | inv_mv | inv_proj], [B,16] each, contract layout (written by k_project_verts)
    int* seed;    // tet: ray_random_seed of the forward (the backward recomputes the same jittered rays)
    // tri: coverage masks the forward keeps for the backward: one 4 KB slot (256 pixels x 128 face bits) per 128-entry chunk of a
    // tile's list.  Chunk 0 of the tile at position q of tile_order (busy tiles come first there: q < number of busy tiles
    // <= min(tiles, list entries)) is slot q of the first mask_first_slots() slots; chunk c >= 1 of a list that starts at entry
    // `begin` is slot mask_first_slots() + begin / 128 + c - 1 (the next busy tile's chunks start at or behind
    // (begin + len) / 128 >= begin / 128 + ceil(len / 128) - 1: no two chunks share a slot).  So the masks grow with the list
    // entries, not with the tiles of the frame (up to round 2: one slot per tile, empty or not -- 4 GiB for a frame of 1 M
    // tiles).  They live in the binning buffer behind the lists, whose capacity the backward does not know on the host
    // (speculative sizing): mask_offset[0] = their byte offset, mask_offset[1] = mask_first_slots(), kept on the device
    // (written by the scatter pass).
    unsigned long long* mask_offset;
    TetSeq* seq;  // tet: the march sequence's descriptor (below)
};
struct BinningState {
    uint64_t* keys; uint32_t* face_list; uint32_t capacity; unsigned long long mask_offset, mask_first;
    char* base; unsigned long long seq_offset; uint32_t seq_steps;  // tet: the march sequence's region
};
// The four scratch buffers of a call (null buffers: sizes only, null pointers).  The binning buffer as the backward passes and
// dmr_export see it: its lists of R entries (run_forward carves the forward's, with its capacity, itself).
struct Scratch { PointState ps; FaceState fs; ImageState is; BinningState bs; size_t point_bytes, face_bytes, image_bytes; };
// Every launcher below: (the scene, the call's Dims and Scratch, what is this launch's own, the stream).

// ---- binning (dmr_binning.hip)
// A tile's list is [tile_offset[t], tile_end[t]): tile_end is the tile's cursor after the entries were emitted.  Behind the exact
// path (set-up -> scan -> scatter) that is tile_offset[t + 1]; behind the speculative one (launch_bin_faces) the list fills
// only a part of its segment [tile_offset[t], tile_offset[t + 1]), and a cursor BEHIND the segment's end marks a list that did
// not fit: nothing of it can be trusted, the tile counts as empty (the call is redone or its overflow flagged).
__host__ __device__ inline uint32_t list_end(const uint32_t* tile_offset, const uint32_t* tile_end, int tile) {
    const uint32_t e = tile_end[tile];
    return e > tile_offset[tile + 1] ? tile_offset[tile] : e;
}
// Speculative placement: what k_project_verts copies into the call's image buffer (start: ntiles + 1 segment starts in tile
// order, order: the tiles in the placed order of dmr_tile_order.hpp -- blocks of neighbouring tiles per XCD class, longest
// list first inside a class; both persistent, dmr_api.hip).  start == null: nothing.
// (the launcher fills in the image buffer's three arrays and the tile count)
struct SegInit { const uint32_t* start; const uint32_t* order; uint32_t* tile_offset; uint32_t* tile_cursor; uint32_t* tile_order; uint32_t ntiles; };
constexpr SegInit NO_SEGMENTS{nullptr, nullptr, nullptr, nullptr, nullptr, 0u};
constexpr uint32_t SEG_SLACK = 32;  // entries every segment has room for beyond its last count + 25 %: the first row of faces of a
                                  // silhouette that moves into a tile that was empty (12 B each: 3 MB at 8 192 tiles)
// also zeroes the image buffer's counters (tile_count | tile_hits | tile_bound | scan_tmp's buckets: contiguous, a slice per block)
void launch_project_verts(const dmr_scene& s, const Dims& d, const Scratch& c, SegInit seg, hipStream_t st);
void launch_setup_faces(const dmr_scene& s, const Dims& d, const Scratch& c, bool tet, hipStream_t st);
// scan_tmp: scan_tmp_words(ntiles) u32 of scratch whose first SCAN_TMP_BUCKETS words are zero on entry
constexpr int SCAN_TMP_BUCKETS = 128;
size_t scan_tmp_words(int ntiles);
// A size the host waits for travels as ONE 8-byte word in pinned (coherent) host memory: the call's sequence number in the
// top 24 bits, the size (clamped to 40 bits) below.  The host polls the word until the sequence number is its own: no event
// packet in the stream (an event record between two kernels costs the device 2-7 us, profiles/r03/dead_ends.md), no ordering
// question between a value and a flag.
__host__ __device__ inline unsigned long long host_size_word(uint32_t seq, unsigned long long size) {
    return ((unsigned long long)(seq & 0xffffffu) << 40) | (size < (1ull << 40) ? size : (1ull << 40) - 1ull);
}
// the forward behind launch_bin_faces sets this bit of the size it publishes when a tile's entries did not fit its segment (R < 2^31 lies below)
constexpr unsigned long long SIZE_WORD_OVERFLOW = 1ull << 39;
// THE SIZE PORT: where the kernel that computes a size the host may wait on -- R of the tile scans and of the forward's size
// workgroup, the record total of k_scan_hits / k_tri_backward_pix -- publishes it.  sized() (dmr_api.hip) fills one in per call
// and the launchers hand it through by value; publish() is the only device code that forms a size word or touches the
// overflow word.
//   host      pinned word of a default (waiting) call, null otherwise: receives host_size_word(seq, size) in ONE 8-byte
//             store, with SIZE_WORD_OVERFLOW or-ed in when a list left its segment (the host then redoes the call);
//   overflow  pinned sticky word of an asynchronous / captured call, which never reads the size on the host, null otherwise:
//             set to 1 when the size exceeds `capacity` or a segment overflowed; only dmr_overflowed() clears it;
//   NOWHERE   publishes nothing: a redo, whose size is known -- a late store could land in the word after a later call, on
//             another stream, took it over.
// The device-side totals (*num_rendered, an int; *hit_total, 64 bits) are plain stores at their sites, not part of the port.
struct SizeOut {
    unsigned long long* host; uint32_t* overflow; uint32_t seq; uint32_t capacity;
    __device__ __forceinline__ void publish(unsigned long long size, bool segment_overflow = false) const {
        if (host) *host = host_size_word(seq, size | (segment_overflow ? SIZE_WORD_OVERFLOW : 0ull));
        if (overflow && (size > (unsigned long long)capacity || segment_overflow)) *overflow = 1u;
    }
};
constexpr SizeOut NOWHERE{nullptr, nullptr, 0u, 0xffffffffu};
// out: where R goes (the size port above)
void launch_scan_tiles(const Dims& d, const Scratch& c, SizeOut out, hipStream_t st);
// masks: also leaves the coverage masks' place in the image buffer (ImageState::mask_offset; tri)
void launch_scatter_faces(const dmr_scene& s, const Dims& d, const Scratch& c, bool masks, hipStream_t st);
// One kernel in place of set-up, scan and scatter (tri, up to SCAN_SINGLE_MAX tiles): the set-up pass's per-face work and the
// scatter pass's emission (the same code, dmr_binning.hip), a slot being good below min(seg[t + 1], capacity) instead of the
// capacity.  seg = the call's tile_offset, which k_project_verts filled from a placement together with the cursors (SegInit).
// Also writes key_depth and tiles_touched (not face_rect, not tile_count).
// Nothing is summed here: R and the overflow come from the cursors, launch_tri_forward's ListSize.  (The first version let every
// workgroup add its entries to one word and take a ticket, the last one publishing R: 55 us at C4 by the stage events, against
// 39 us for set-up + scan + scatter, profiles/r05/bench_ab_c4_ticket_variant.txt.)
void launch_bin_faces(const dmr_scene& s, const Dims& d, const Scratch& c, hipStream_t st);
// start[ntiles + 1], order[ntiles] <- the placement for the counts (and order) of a call that went through launch_scan_tiles
void launch_build_placement(int ntiles, const uint32_t* tile_count, const uint32_t* tile_order, uint32_t* start, uint32_t* order,
                            hipStream_t st);
// capacity: entries the binning buffer holds; it is below R only while a size guess is being refuted (dmr_api.hip):
// every kernel that walks the tile lists clamps to it, the results are then thrown away and redone.
// Who sorts a tile's list: up to SCAN_SINGLE_MAX tiles the tri forward / the tet first-hit kernel, each tile's workgroup its own
// at its start (they get the unsorted keys); above, launch_sort_tiles ahead of them (and they get no keys).
inline bool sorts_own_tiles(const Dims& d) { return d.ntiles <= SCAN_SINGLE_MAX; }
void launch_sort_tiles(const Dims& d, const Scratch& c, hipStream_t st);

// ---- tri compositing (dmr_tri.hip)
constexpr int MASK_CHUNK = 128;     // list entries per mask slot = the compositing kernels' chunk
inline size_t mask_first_slots(size_t list_capacity, size_t ntiles) { return list_capacity < ntiles ? list_capacity : ntiles; }
inline size_t mask_slots(size_t list_capacity, size_t ntiles) { return mask_first_slots(list_capacity, ntiles) + list_capacity / MASK_CHUNK + 1; }
// One blended (pixel, face) pair, written face-major per (tile, chunk, pass) by k_tri_backward_pix and
// consumed one per lane by k_tri_backward_hits.
// (A 32-byte record carrying face and vertex ids was tried: kernel 2 did not get faster, kernel 1 got 9 % slower.)
struct alignas(16) HitRecord { uint32_t id; uint32_t pixel; float T; float dL_dalpha; };  // id: word (slot mod HIT_GROUP) of {face, v0, v1, v2}; pixel: tile-local
// alpha (DMR_FLAG_ALPHA, every launcher that takes it): the depth image -- out_depth, dL_ddepth -- has two channels, [B,2,H,W]:
// channel 0 the depth, channel 1 the accumulated opacity alpha = 1 - T_final (0 where a tet pixel's march fails) / its
// upstream gradient, which reaches dL_dfopacity only.  A compile-time variant of the kernels; the default ones are unchanged.
// sorts_own_tiles(): the kernel gets the unsorted (depth_bits << 32 | face) list entries of the scatter pass (BinningState::keys)
// and every tile's workgroup sorts its own list (dmr_sort.hpp) into face_list before compositing it; else face_list is sorted already
// size (blocks = 1: behind launch_bin_faces, which sums nothing): one more workgroup adds up the lists, stores R and publishes
// it through the size port -- with the segment-overflow flag if a list left its segment -- as launch_scan_tiles does on the
// exact path
struct ListSize { int* num_rendered; SizeOut out; uint32_t blocks; };
// The fragment lists of either renderer (DMR_FLAG_TRI_FRAGMENTS / DMR_FLAG_TET_FRAGMENTS): K slots per pixel, 1 <= K <=
// FRAG_MAX_K, in the caller's ONE buffer [face i32 B,K,H,W | bary f32 B,K,2,H,W | count i32 B,H,W] of npix = B H W pixels.
// The inputs of the gradient flags: face as above, the gradient of bary in its layout.
constexpr int FRAG_MAX_K = 32;
struct FragmentLists {
    int32_t* face; float* bary; int32_t* count;
    FragmentLists(void* buf, size_t npix, int K)
        : face(static_cast<int32_t*>(buf)), bary(reinterpret_cast<float*>(face + (size_t)K * npix)), count(face + 3 * (size_t)K * npix) {}
    static size_t bytes(size_t npix, int K) { return 4 * npix * (3 * (size_t)K + 1); }
    static size_t face_bytes(size_t npix, int K) { return 4 * npix * (size_t)K; }
    static size_t bary_bytes(size_t npix, int K) { return 8 * npix * (size_t)K; }
};
constexpr ListSize NO_LIST_SIZE{nullptr, NOWHERE, 0u};
void launch_tri_forward(const dmr_scene& s, const Dims& d, const Scratch& c, float* out_color, float* out_depth, bool alpha,
                        ListSize size, hipStream_t st);
// DMR_FLAG_TRI_FRAGMENTS, behind the call's final launch_tri_forward (whose state it reads: sorted lists, coverage masks,
// n_contrib): per pixel of the band the first K blended (pixel, face) pairs in blend order and their number, into the
// caller's buffer (FragmentLists; bary: (u_c, v_c); unused slots -1 / 0).
// No stage of its own, no size, no host wait.
void launch_tri_fragments(const dmr_scene& s, const Dims& d, const Scratch& c, int K, void* fragments, hipStream_t st);
// hit_offset: every tile's region of the record buffer, sized by the bound h + (HIT_GROUP - 1) * min(list length, h) of
// its h blended pairs (tile_hits); tile_used is cleared (the per-pixel kernel fills it).  out: where the total goes (size port)
void launch_scan_hits(const Dims& d, const Scratch& c, SizeOut out, hipStream_t st);
// Without launch_scan_hits (B * tiles <= SCAN_SINGLE_MAX): every workgroup of k_tri_backward_pix sums the record bounds of
// the tiles before its own (tile_bound: eight 16-byte loads per thread, all in flight at once) and publishes hit_offset[tile] /
// tile_used[tile] for the hit-parallel kernel; the last tile's workgroup also stores the total and publishes it through the
// size port.  One launch and ~8 us of single-workgroup latency less per step.
struct HitRegions {
    uint32_t* hit_offset;                 // null: the regions come from launch_scan_hits
    unsigned long long* hit_total;
    SizeOut out;
};
// also zeroes work[0, work_floats) (the packed accumulators)
// capacity (here and in launch_tri_backward_hits): records `hits` holds
void launch_tri_backward_pix(const dmr_scene& s, const Dims& d, const Scratch& c, const float* dL_dcolor, const float* dL_ddepth,
                             float4* pixrec, HitRecord* hits, uint32_t capacity, float* work, size_t work_floats,
                             HitRegions regions, bool alpha, hipStream_t st);
// one workgroup per tile (longest list first) over the tile's tile_used records.
// grads: the vertex-position gradient the kernel forms -- TRI_GRAD_REF the reference's ray_tri_intersection_grad (Q11),
// TRI_GRAD_EXACT the exact derivative of each pair's (u, v), TRI_GRAD_CAMERA that and the ray's: every tile of the call
// then stores its 32-float part of [dL/dinv_mv 16 | dL/dinv_proj 16] (contract layout) at cam_part + 32 * tile (tiles
// that blend nothing keep what is there: the zeros of k_tri_backward_pix, which clears cam_part with the accumulators)
enum { TRI_GRAD_REF = 0, TRI_GRAD_EXACT = 1, TRI_GRAD_CAMERA = 2 };
void launch_tri_backward_hits(const dmr_scene& s, const Dims& d, const Scratch& c, const float4* pixrec, const HitRecord* hits,
                              uint32_t capacity, float* vrow, float* frow, int grads, float* cam_part, hipStream_t st);
// DMR_FLAG_TRI_FRAGMENT_GRADS, behind launch_tri_backward_hits and ahead of the unpack / launch_camera_reduce: for every pixel of
// the band and each of its K slots, dL/d(u_c, v_c) (frag_grad, f32 [B,K,2,H,W]) of the pair (pixel, frag_face[slot], i32
// [B,K,H,W]) through the clamp and the exact derivative of the pair's (u, v) (PairUV, dmr_device.hpp), added into the position
// columns of the packed vertex rows and, cam_part != null, into every tile's 32-float camera partial (ray_chain).  A face outside
// [0, F) is no pair.  Reads the scene, the contract-layout inverse matrices and the two inputs only.  No stage of its own, no
// size, no host wait.
void launch_tri_fragment_grads(const dmr_scene& s, const Dims& d, const Scratch& c, int K, const int32_t* frag_face,
                               const float* frag_grad, float* vrow, float* cam_part, hipStream_t st);
// sums the B * tiles partials of a camera variant per view, in a fixed order: out [B][width]; width 32 (the tri
// renderer's, see launch_tri_backward_hits) or 64 (the tet renderer's, see launch_tet_backward)
void launch_camera_reduce(int B, int tiles, int width, const float* cam_part, float* out, hipStream_t st);
void launch_tri_unpack(const dmr_scene& s, const float* vrow, const float* frow, float* dL_dverts,
                       float* dL_dvcolor, float* dL_dfopacity, float* dL_dvdepth, float* dL_dfintense,
                       hipStream_t st);

// ---- tet ray march (dmr_tet.hip)
// The MARCH SEQUENCE the forward leaves for the backward: the faces every pixel crossed, in order, so that the backward
// consumes them from the back instead of re-discovering them (the reference re-marches: three ray-triangle tests and four
// outward normals per step, cuda_renderer/backward.cu:372-476).  Static layout, no allocation on the device: wave w of the
// forward (tile * 4 + quadrant; its 64 pixels are at the same step in the same loop iteration) owns cap_steps / 4 rows of
// 64 x 16 bytes, step s of lane l is dword (s & 3) of the 16-byte word l of row s / 4 -- a lane stores four steps as one
// 16-byte word, a wave's store / load of a row is one contiguous kilobyte.  The region lies in the binning buffer behind
// the lists; cap_steps is the longest march of the previous call with the same view configuration + 25 % (dmr_api.hip; a
// dynamic allocation of 4-KB chunks from an atomic counter was measured first: its bookkeeping inside the march loop cost
// the forward 100 us at C3, more than the backward gained).  A sequence that did not fit (max_steps > cap_steps; cap_steps
// == 0: no estimate yet) is ignored: the backward then re-marches like the reference.
// Its second reader is k_tet_fragments (DMR_FLAG_TET_FRAGMENTS), which takes the first K entries of every pixel: a forward
// with that flag has cap_steps >= K rounded up to 4 whatever the estimate (dmr_api.hip), and those entries are there whether
// or not the whole sequence fits.
// Bit 31 of an entry: the reference's reverse march would stop behind this face ("error case 3": a second face of the
// tet the ray leaves through this one is hit from outside as well, backward.cu:456-460) -- the forward has those three
// tests in its hands anyway, so the backward reproduces the reference's decision without repeating them.
struct TetSeq {
    uint32_t max_steps;         // longest march of this forward (atomicMax, one per wave): complete iff <= cap_steps
    uint32_t cap_steps;         // steps per pixel the region has room for (a multiple of 4; 0: no region)
    unsigned long long offset;  // bytes from the binning buffer's start
};
inline size_t tet_seq_bytes(size_t ntiles, size_t cap_steps) { return ntiles * 4 * (cap_steps / 4) * 1024; }
size_t tet_facerec_bytes();   // per face
size_t tet_colrec_bytes();    // per face
size_t tet_tetrec_bytes();    // per tet
// builds the packed march records from the scene (every forward call); also resets the march sequence's descriptor:
// room for BinningState::seq_steps steps per pixel at byte seq_offset of the binning buffer
void launch_tet_prep(const dmr_scene& s, const Dims& d, const Scratch& c, hipStream_t st);
// sorts_own_tiles(): as launch_tri_forward (every tile's workgroup sorts its list itself)
void launch_tet_first_intersect(const dmr_scene& s, const Dims& d, const Scratch& c, hipStream_t st);
void launch_tet_forward(const dmr_scene& s, const Dims& d, const Scratch& c, float* out_color, float* out_depth, float* out_active,
                        bool alpha, hipStream_t st);
// DMR_FLAG_TET_FRAGMENTS, behind the call's final launch_tet_forward (whose state it reads: n_contrib, is_active and the march
// sequence, which such a call sizes to at least K steps rounded up to 4): per pixel of the band the first K faces the march
// composited, front to back, the (u, v) of the pixel's ray on each and their number, into the caller's buffer (FragmentLists;
// unused slots -1 / 0; count = n_contrib where is_active, else 0).  No stage of its own, no size, no host wait.
void launch_tet_fragments(const dmr_scene& s, const Dims& d, const Scratch& c, int K, void* fragments, hipStream_t st);
void launch_tet_zero_grads(float* dL_dvcolor, int64_t n_vcolor, float* dL_dfopacity, int64_t n_fopacity, hipStream_t st);
// Two launches, of which the device runs one: k_tet_backward_seq when the forward's march sequence is complete
// (seq->max_steps <= seq->cap_steps != 0), else the re-marching k_tet_backward; the other one returns at once.  No host read.
// host_seq_steps (pinned, may be null): receives seq->max_steps, the next forward's capacity estimate.
// dL_dverts, dL_dfintense: the full gradients (null: the default kernels).  cam_part (needs them): the camera variant,
// which also stores every tile's 64-float partial [dL/dinv_mv | dL/dinv_proj | dL/dmv | dL/dproj] (contract layout) at
// cam_part + 64 * ((view * (r1 - r0) + row - r0) * gx + column) -- launch_camera_reduce's input with tiles = gx (r1 - r0).
void launch_tet_backward(const dmr_scene& s, const Dims& d, const Scratch& c, const float* dL_dcolor, const float* dL_ddepth,
                         float* dL_dvcolor, float* dL_dfopacity, uint32_t* host_seq_steps, float* dL_dverts, float* dL_dfintense,
                         float* cam_part, bool alpha, hipStream_t st);
// DMR_FLAG_TET_FRAGMENT_GRADS, behind launch_tet_backward (which zeroed and filled dL_dverts and stored every band tile's cam_part)
// and ahead of launch_camera_reduce: for every pixel of the band and each of its K slots, dL/d(u, v) (frag_grad, f32
// [B,K,2,H,W]) of the pair (pixel, frag_face[slot], i32 [B,K,H,W]) through the exact derivative of the pair's unclamped (u, v) on
// the forward's ray (PairUV, dmr_device.hpp), added into dL_dverts [P,3] and, cam_part != null, into the first 32 floats
// (dL/dinv_mv | dL/dinv_proj) of every tile's 64-float camera partial (ray_chain).  A face outside [0, F) is no pair.  Reads the
// scene, the face records and the seed the forward left, the contract-layout inverse matrices and the two inputs only.  No stage
// of its own, no size, no host wait.
void launch_tet_fragment_grads(const dmr_scene& s, const Dims& d, const Scratch& c, int K, const int32_t* frag_face,
                               const float* frag_grad, float* dL_dverts, float* cam_part, hipStream_t st);

}  // namespace dmr
