// dmr_api.hip -- C ABI (include/dmesh_renderer_amd.h) and host orchestration.
//
// Replaces the host side of Rasterizer::forward/backward (cuda_rasterizer/rasterizer_impl.cu:175-467)
// and Renderer::forward/backward (cuda_renderer/renderer_impl.cu:193-498): scratch carving,
// stage sequencing, the single device->host read of num_rendered.  Unlike the reference
// (a cudaDeviceSynchronize after every stage on the legacy default stream, Q14) everything is
// enqueued on the caller's stream and the only host wait is that 4-byte read, which sizes the
// binning buffer.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "dmr_kernels.hpp"
#include "dmr_placement_key.hpp"
#include "dmr_tile_order.hpp"

namespace {

thread_local std::string g_err;

int fail(const std::string& m) { g_err = m; return 1; }

#define DMR_HIP(expr)                                                                           \
    do {                                                                                        \
        hipError_t e_ = (expr);                                                                 \
        if (e_ != hipSuccess) return fail(std::string(#expr) + ": " + hipGetErrorString(e_));   \
    } while (0)

// An output the caller provides through `alloc` (the DMR_BUF_* ids beyond the work space), requested once; not at all when
// bytes == 0 (flag not set, or an empty output).  idle: nothing to back-propagate: zeroed here, and *out stays null.
int caller_output(dmr_alloc_fn alloc, void* ctx, int which, size_t bytes, const char* what, bool idle, hipStream_t st, float** out) {
    *out = nullptr;
    if (bytes == 0) return 0;
    if (!alloc) return fail("null argument");
    float* p = static_cast<float*>(alloc(ctx, which, bytes));
    if (!p) return fail(std::string("allocation of the ") + what + " buffer failed");
    if (idle) DMR_HIP(hipMemsetAsync(p, 0, bytes, st));
    else *out = p;
    return 0;
}

// K of a call, the fragment slots per pixel in bits 8-15 of the flags, when `flag` (one of the four fragment flags, `name`;
// `macro`: what the header offers for those bits) is set, else 0.  -1, with the error set: K outside 1..FRAG_MAX_K.
int fragment_k(const dmr_scene* s, int flag, const char* name, const char* macro) {
    const int K = (s->flags & flag) ? DMR_FRAGMENTS_K(s->flags) : 0;
    if ((s->flags & flag) && (K < 1 || K > dmr::FRAG_MAX_K))
        return -fail(std::string(name) + ": K (bits 8-15 of flags, " + macro + ") must be in 1..32, got " + std::to_string(K));
    return K;
}

// The two inputs of a fragment-gradient call, the caller's face and bary-gradient buffers, requested once each.  r / R: the
// renderer in the messages, "tri" / "TRI" or "tet" / "TET".
int fragment_grad_inputs(dmr_alloc_fn alloc, void* ctx, const char* r, const std::string& R, int face_id, int grad_id, size_t npix, int K,
                         const int32_t** face, const float** grad) {
    if (!alloc) return fail("null argument");
    const std::string no = "DMR_FLAG_" + R + "_FRAGMENT_GRADS: no " + r + " fragment ";
    *face = static_cast<const int32_t*>(alloc(ctx, face_id, dmr::FragmentLists::face_bytes(npix, K)));
    if (!*face) return fail(no + "face buffer (DMR_BUF_" + R + "_FRAGMENT_FACES)");
    *grad = static_cast<const float*>(alloc(ctx, grad_id, dmr::FragmentLists::bary_bytes(npix, K)));
    if (!*grad) return fail(no + "bary gradient buffer (DMR_BUF_" + R + "_FRAGMENT_BARY_GRADS)");
    return 0;
}

using dmr::Dims;  // a call's scratch, as the launchers see it: dmr_kernels.hpp
using dmr::PointState;
using dmr::FaceState;
using dmr::ImageState;
using dmr::BinningState;
using dmr::Scratch;

constexpr size_t ALIGN = 256;
inline size_t up(size_t n) { return (n + ALIGN - 1) & ~(ALIGN - 1); }

// Bump carving of a scratch buffer (the reference's obtain(), rasterizer_impl.h:10-16).
struct Carver {
    char* base; size_t off;
    explicit Carver(void* b) : base(reinterpret_cast<char*>(b)), off(0) {}
    template <class T> T* take(size_t count) {
        T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off += up(count * sizeof(T));
        return p;
    }
};

size_t carve_point(void* b, size_t BP, PointState& s) { Carver c(b); s.vproj = c.take<float4>(BP); return c.off; }
size_t carve_face(void* b, size_t BF, size_t F, size_t T, bool tet, FaceState& s) {
    Carver c(b);
    s.rect = c.take<uint2>(BF); s.key_depth = c.take<float>(BF);
    s.max_depth = tet ? c.take<float>(BF) : nullptr;
    s.tiles_touched = c.take<uint32_t>(BF);
    s.facerec = s.colrec = s.tetrec = nullptr;
    if (tet) {  // packed march records (view independent)
        s.facerec = c.take<char>(F * dmr::tet_facerec_bytes());
        s.colrec = c.take<char>(F * dmr::tet_colrec_bytes());
        s.tetrec = c.take<char>(T * dmr::tet_tetrec_bytes());
    }
    return c.off;
}
size_t carve_image(void* b, size_t B, size_t ntiles, size_t npix, bool tet, ImageState& s) {
    Carver c(b);
    s.mats = c.take<float>(64 * B);
    s.seed = c.take<int>(1);
    s.mask_offset = c.take<unsigned long long>(2);
    // counters, zeroed by k_project_verts at the start of a forward: [tile_count | tile_hits | tile_bound | scan_tmp's buckets]
    s.tile_count = c.take<uint32_t>(ntiles); s.tile_hits = c.take<uint32_t>(ntiles); s.tile_bound = c.take<uint32_t>(ntiles);
    s.scan_tmp = c.take<uint32_t>(dmr::scan_tmp_words((int)ntiles));
    s.hit_offset = c.take<uint32_t>(ntiles + 1); s.tile_used = c.take<uint32_t>(ntiles); s.hit_total = c.take<unsigned long long>(1);
    s.tile_offset = c.take<uint32_t>(ntiles + 1);
    s.tile_cursor = c.take<uint32_t>(ntiles); s.num_rendered = c.take<int>(1);
    s.tile_order = c.take<uint32_t>(ntiles);
    s.final_T = c.take<float>(npix); s.final_prev_T = c.take<float>(npix); s.n_contrib = c.take<uint32_t>(npix);
    if (tet) {
        s.first_face = c.take<int32_t>(npix); s.first_tet = c.take<int32_t>(npix);
        s.last_face = c.take<int32_t>(npix); s.last_tet = c.take<int32_t>(npix);
        s.is_active = c.take<uint8_t>(npix);
        s.seq = c.take<dmr::TetSeq>(1);
    } else {
        s.first_face = s.first_tet = s.last_face = s.last_tet = nullptr; s.is_active = nullptr;
        s.seq = nullptr;
    }
    return c.off;
}
// face_list first: the backward re-derives it from the buffer start, whatever capacity the forward
// gave the buffer (speculative sizing allocates more than R entries)
// ... then, tri only, the coverage masks the forward leaves for the backward (dmr_kernels.hpp): their place depends on the
// capacity, so the kernels take it from the device (ImageState::mask_offset, written by the scatter pass).  mask_tiles = 0:
// no masks (tet; the backward, which never carves beyond the lists on the host).
// ... or, tet only, the forward's march sequence (seq_steps steps per pixel of seq_tiles tiles, dmr_kernels.hpp; its place is
// kept on the device too).
size_t carve_binning(void* b, size_t R, size_t mask_tiles, size_t seq_tiles, size_t seq_steps, BinningState& s) {
    Carver c(b);
    s.face_list = c.take<uint32_t>(R); s.keys = c.take<uint64_t>(R);
    s.capacity = (uint32_t)std::min<size_t>(R, 0xffffffffu);
    s.mask_offset = c.off;
    s.mask_first = dmr::mask_first_slots(R, mask_tiles);
    if (mask_tiles && R > 0) c.take<uint4>(dmr::mask_slots(R, mask_tiles) * 256);
    s.base = reinterpret_cast<char*>(b); s.seq_offset = c.off; s.seq_steps = (uint32_t)seq_steps;
    if (seq_steps) c.take<char>(dmr::tet_seq_bytes(seq_tiles, seq_steps));
    return c.off;
}

// The four scratch buffers of a call (dmr::Scratch; null buffers: sizes only, null pointers), the binning buffer's lists of R
// entries included.
Scratch carve_scratch(const dmr_scene* s, bool tet, const Dims& d, const void* pb, const void* fb, const void* ib,
                      const void* bb = nullptr, size_t R = 0) {
    Scratch c;
    c.point_bytes = carve_point(const_cast<void*>(pb), d.BP, c.ps);
    c.face_bytes = carve_face(const_cast<void*>(fb), d.BF, (size_t)s->F, (size_t)s->T, tet, c.fs);
    c.image_bytes = carve_image(const_cast<void*>(ib), (size_t)s->B, (size_t)d.ntiles, d.npix, tet, c.is);
    carve_binning(const_cast<void*>(bb), R, 0, 0, 0, c.bs);
    return c;
}
// The scene as every kernel behind k_project_verts sees it: matrices in contract layout, read from the image buffer.
dmr_scene canonical(const dmr_scene* s, const float* mats) {
    dmr_scene c = *s;
    const size_t n = 16 * (size_t)s->B;
    c.mv_mats = mats; c.proj_mats = mats + n; c.inv_mv_mats = mats + 2 * n; c.inv_proj_mats = mats + 3 * n;
    c.mats_transposed = 0;
    return c;
}

int check_scene(const dmr_scene* s, bool tet, Dims& d) {
    if (!s) return fail("null scene");
    if (s->B <= 0 || s->W <= 0 || s->H <= 0 || s->P < 0 || s->F < 0 || s->T < 0) return fail("bad dimensions");
    if ((int64_t)s->B * s->P > INT32_MAX || (int64_t)s->B * s->F > INT32_MAX || (int64_t)s->B * s->W * s->H > INT32_MAX)
        return fail("problem too large for 32-bit indexing");
    d.gx = (s->W + dmr::TILE - 1) / dmr::TILE;
    d.gy = (s->H + dmr::TILE - 1) / dmr::TILE;
    if (d.gx > 65535 || d.gy > 65535) return fail("image too large (tile coordinates must fit 16 bits)");
    d.r0 = s->row_begin; d.r1 = s->row_end;
    if (d.r0 == 0 && d.r1 == 0) d.r1 = d.gy;
    d.r0 = std::max(0, std::min(d.gy, d.r0));
    d.r1 = std::max(d.r0, std::min(d.gy, d.r1));
    d.ntiles = s->B * d.gx * d.gy;
    d.BP = (size_t)s->B * s->P; d.BF = (size_t)s->B * s->F; d.npix = (size_t)s->B * s->W * s->H;
    if (tet && s->F > 0 && s->P > 0 && (!s->tets || !s->face_tets || !s->tet_faces)) return fail("tet topology missing");
    if (tet && s->F >= (1 << 28)) return fail("too many faces for the tet renderer (face ids must fit 28 bits)");
    return 0;
}

// 64 zeroed bytes of pinned (coherent, device-visible) host memory for words the kernels store into; null: failed
void* pinned_words() {
    void* p = nullptr;
    if (hipHostMalloc(&p, 64, hipHostMallocCoherent | hipHostMallocPortable) != hipSuccess) return nullptr;
    memset(p, 0, 64);
    return p;
}

// Pinned landing pad the kernels write the sizes to -- forward: the 8-byte word at byte 0, backward: the one at byte 8, each
// host_size_word(sequence number, size) (dmr_kernels.hpp) -- one per host thread and device.  The host POLLS the word until it
// carries the call's sequence number: an event recorded between two kernels costs the device 2-7 us
// (profiles/r03/dead_ends.md), a default call had two of them per step.
struct SizeRead {
    void* slot = nullptr; uint32_t seq = 0;
    volatile unsigned long long* word(int which) const { return reinterpret_cast<volatile unsigned long long*>(slot) + which; }
    uint32_t next_seq() { seq = (seq + 1u) & 0xffffffu; if (seq == 0u) seq = 1u; return seq; }
};
thread_local std::map<int, SizeRead> g_size_read;  // per device
// Waits until *w carries `seq`; returns the size in it.  Spins on the pinned word; if it does not arrive within ~50 ms the
// stream is synchronised instead (a kernel error then surfaces as a HIP error, and a completed stream has written the word).
int wait_size(volatile unsigned long long* w, uint32_t seq, hipStream_t st, unsigned long long* size) {
    const auto t0 = std::chrono::steady_clock::now();
    for (uint32_t spins = 0;; spins++) {
        const unsigned long long v = *w;
        if ((uint32_t)(v >> 40) == (seq & 0xffffffu)) { std::atomic_thread_fence(std::memory_order_acquire); *size = v & ((1ull << 40) - 1ull); return 0; }
        if ((spins & 1023u) == 1023u && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(50)) break;
#if defined(__x86_64__) || defined(__i386__)
        __builtin_ia32_pause();
#endif
    }
    DMR_HIP(hipStreamSynchronize(st));
    const unsigned long long v = *w;
    if ((uint32_t)(v >> 40) != (seq & 0xffffffu)) return fail("the size word was not written (internal error)");
    *size = v & ((1ull << 40) - 1ull);
    return 0;
}

// Sticky per-device overflow word of the asynchronous / captured calls (pinned host memory the scan kernels store 1
// into when a scene outgrew the capacity a call was enqueued with); read by dmr_overflowed().  Created by the first
// default (waiting) call on a device -- never inside a stream capture, where hipHostMalloc is not allowed.
std::mutex g_overflow_mu;
std::map<int, uint32_t*> g_overflow;
uint32_t* overflow_word(int dev, bool create) {
    std::lock_guard<std::mutex> lk(g_overflow_mu);
    auto it = g_overflow.find(dev);
    if (it != g_overflow.end()) return it->second;
    if (!create) return nullptr;
    void* p = pinned_words();
    if (!p) return nullptr;
    return g_overflow[dev] = reinterpret_cast<uint32_t*>(p);
}

// DMR_FLAG_ASYNC, or a stream being captured into a HIP graph: the call must not wait for the device
bool is_async(const dmr_scene* s, hipStream_t st) {
    if (s->flags & DMR_FLAG_ASYNC) return true;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) != hipSuccess) { (void)hipGetLastError(); return false; }
    return cs != hipStreamCaptureStatusNone;
}

// Speculative sizing.  The sizes of the binning buffer (R) and of the hit-record buffer are
// only known on the device.  The reference stalls the pipeline on a device->host read before it can continue
// (rasterizer_impl.cu:287-299).  Here the previous call with the same view configuration provides a capacity guess
// (its sizes per face / per list entry, +25 %): the buffer is allocated and ALL remaining kernels are enqueued
// before the host waits -- and it waits for the word the size-writing kernel stores into pinned host memory (polled: no
// event packet, no stream synchronisation), so the GPU keeps running.  Kernels clamp their writes to the capacity; if
// the exact size turns out larger the affected stages are simply enqueued again with an exact buffer (first call,
// or a scene that grew by more than 25 %).
// The guess is keyed by the view configuration only and kept as RATIOS (list entries and hit records per (view, face)
// pair): a mesh whose face count changes every iteration (DMesh re-tetrahedralises) still gets a guess, and the cache
// stays a handful of entries.
// Asynchronous calls (DMR_FLAG_ASYNC, or a stream that is being captured into a HIP graph) use the same estimate and
// never wait: the size is not read back at all, the scan kernel compares it with the capacity on the device and sets
// the sticky overflow word (dmr_overflowed).  That is what makes forward + backward capturable as one graph.
struct SizeKey {
    int v[7];
    bool operator<(const SizeKey& o) const { return memcmp(v, o.v, sizeof(v)) < 0; }
};
// seq_steps: tet only -- pinned word the backward kernels leave the forward's longest march in (steps); read without any
// wait by the next forward as its capacity estimate (a stale value only costs that call the re-marching backward)
struct SizeGuess { double rendered_per_face = 0.0, hits_per_face = 0.0; uint32_t* seq_steps = nullptr; };
std::mutex g_size_mu;
std::map<SizeKey, SizeGuess> g_size_cache;
// ... and by the magnitude of the mesh (floor(log2(B * F))): two renderers with the same view configuration and meshes of very
// different size -- say a coarse and a fine level of one pipeline, alternating -- would otherwise trade one entry back and forth
// between over-allocation and the redo path ("what's weak" 8).  A mesh that crosses a power of two finds the
// neighbouring bucket's estimate (lookup tries b, b - 1, b + 1).
std::atomic<uint64_t> g_redo_count{0};  // stages enqueued a second time because an estimate was too small (dmr_redo_count)
int size_bucket(size_t BF) { int b = 0; while ((BF >> (b + 1)) != 0) b++; return b; }
SizeKey size_key(const dmr_scene* s, bool tet, const Dims& d) {
    return SizeKey{{s->B, s->W, s->H, d.r0, d.r1, tet ? 1 : 0, size_bucket(d.BF)}};
}
// the estimate `field` of this key's bucket or, failing that, of a neighbouring bucket (0: none); g_size_mu held
double lookup_estimate(const SizeKey& key, double SizeGuess::* field) {
    for (int db : {0, -1, 1}) {
        SizeKey k = key; k.v[6] += db;
        auto it = g_size_cache.find(k);
        if (it != g_size_cache.end() && it->second.*field > 0.0) return it->second.*field;
    }
    return 0.0;
}
uint64_t padded(uint64_t n) { return n + n / 4 + 4096; }

// Speculative PLACEMENT of the tile segments (tri, single frames up to SCAN_SINGLE_MAX tiles).  The exact path counts every
// (face, tile) pair, scans the counts in one workgroup and visits every face again to scatter: three dependent launches
// whose only purpose is to know where a tile's list starts.  Like the sizes above, that is taken from the previous call of
// the key instead: a default call that went through the exact path (the first one of a key, and every redo) leaves, in
// device memory the library owns, a segment per tile -- room for its count + 25 % + SEG_SLACK entries, in tile order -- and
// its tile order.  Later calls of the key bin in ONE kernel straight into those segments (launch_bin_faces); a tile that
// outgrew its segment raises the overflow bit of the size word (default call: redone through the exact path, which
// refreshes the placement; asynchronous call: the sticky overflow word).  The arrays are allocated once per key and
// rewritten in place, so a captured graph keeps valid addresses; the capacity a graph was captured with bounds every
// store of its replays.  A default call whose R fell below HALF the R the placement was built from drops it: the next
// default call rebuilds it through the exact path (a shrinking scene does not keep a stale order and padding for ever).
struct Placement { uint32_t* start = nullptr; uint32_t* order = nullptr; int ntiles = 0; uint64_t capacity = 0, built_from = 0; bool valid = false; };
// Keyed by DEVICE and view configuration (dmr_placement_key.hpp): the arrays are memory of the device that built them, and a
// device only ever sees arrays it allocated.  g_placement_mu is held over a whole build (allocate, rewrite, publish), so two
// threads' first default calls of one key neither allocate twice nor rewrite arrays the other one is about to hand out; the
// arrays live as long as the process (one pair per key and device).
std::mutex g_placement_mu;
std::map<dmr::PlacementKey, Placement> g_placement;  // g_size_mu
int current_device() { int dev = 0; if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); dev = -1; } return dev; }
dmr::PlacementKey placement_key(const SizeKey& key) { return dmr::placement_key(current_device(), key.v, 7); }
uint64_t placement_capacity(uint64_t R, int ntiles) { return R + R / 4 + (uint64_t)dmr::SEG_SLACK * (uint64_t)ntiles; }  // >= the segments' sum
bool placement_eligible(bool tet, const Dims& d) { return !tet && d.ntiles <= dmr::SCAN_SINGLE_MAX; }
Placement find_placement(const SizeKey& key, const Dims& d) {
    const dmr::PlacementKey pk = placement_key(key);
    if (pk.device < 0) return Placement{};
    std::lock_guard<std::mutex> lk(g_size_mu);
    auto it = g_placement.find(pk);
    return it != g_placement.end() && it->second.valid && it->second.ntiles == d.ntiles ? it->second : Placement{};
}
void drop_placement(const SizeKey& key) {
    const dmr::PlacementKey pk = placement_key(key);
    std::lock_guard<std::mutex> lk(g_size_mu);
    auto it = g_placement.find(pk);
    if (it != g_placement.end()) it->second.valid = false;
}
// From the counts and the order a default call's exact path left in its image buffer (never inside a capture).  Calls of the
// key that are still in flight on other streams read the arrays: the device is drained before they are rewritten, and the
// stream before the next call can use them.
int build_placement(const SizeKey& key, const Dims& d, uint64_t R, const ImageState& is, hipStream_t st) {
    const uint64_t capacity = placement_capacity(R, d.ntiles);
    if (capacity > 0x7fffffffu) { drop_placement(key); return 0; }
    const dmr::PlacementKey pk = placement_key(key);
    if (pk.device < 0) return 0;
    std::lock_guard<std::mutex> build_lk(g_placement_mu);
    Placement p;
    {
        std::lock_guard<std::mutex> lk(g_size_mu);
        p = g_placement[pk];
        g_placement[pk].valid = false;  // nobody takes it up while it is being rewritten
    }
    if (p.start && p.ntiles != d.ntiles) return 0;  // (cannot happen: the key holds B, W, H)
    if (!p.start) {
        void* mem = nullptr;
        DMR_HIP(hipMalloc(&mem, sizeof(uint32_t) * (2 * (size_t)d.ntiles + 1)));
        p.start = reinterpret_cast<uint32_t*>(mem); p.order = p.start + d.ntiles + 1; p.ntiles = d.ntiles;
    } else {
        DMR_HIP(hipDeviceSynchronize());
    }
    dmr::launch_build_placement(d.ntiles, is.tile_count, is.tile_order, p.start, p.order, st);
    // The order placed calls take their tiles in: not the exact path's "longest list first" over the whole frame but the
    // XCD-local one of dmr_tile_order.hpp, from the counts and the blended pairs this call's forward left (host C++: 32 KB
    // each way, once per placement, behind a wait this function needs anyway).  Busy tiles need not come first in it: a
    // placed call's capacity is at least SEG_SLACK entries per tile, so mask_first_slots(capacity, ntiles) == ntiles and
    // every position is a first-chunk mask slot (dmr_kernels.hpp, ImageState::mask_offset).
    static_assert(dmr::SEG_SLACK >= 1, "a placed call's list capacity covers one entry per tile");
    const size_t n = (size_t)d.ntiles;
    std::vector<uint32_t> host(3 * n);
    DMR_HIP(hipMemcpyAsync(host.data(), is.tile_count, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, st));
    DMR_HIP(hipMemcpyAsync(host.data() + n, is.tile_hits, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, st));
    DMR_HIP(hipStreamSynchronize(st));
    dmr::tile_order(d.ntiles / (d.gx * d.gy), d.gx, d.gy,host.data(), host.data() + n, host.data() + 2 * n);
    DMR_HIP(hipMemcpyAsync(p.order, host.data() + 2 * n, sizeof(uint32_t) * n, hipMemcpyHostToDevice, st));
    DMR_HIP(hipStreamSynchronize(st));
    p.capacity = capacity; p.built_from = R; p.valid = true;
    std::lock_guard<std::mutex> lk(g_size_mu);
    g_placement[pk] = p;
    return 0;
}

constexpr uint64_t TET_SEQ_BUDGET = 16ull << 30;  // tet: bytes of march sequence a call may own
// ... and the steps per pixel it has room for (a multiple of 4, at least 4)
uint64_t march_budget_steps(const Dims& d) {
    return std::max<uint64_t>(TET_SEQ_BUDGET / std::max<uint64_t>(dmr::tet_seq_bytes((size_t)d.ntiles, 4), 1), 1) * 4;
}
// tet: the key's SizeGuess::seq_steps word (created by a default forward: create; null: none) and, if asked for, the room for
// the next forward's march sequence: the longest march + 25 %, a multiple of 4, within that budget (0: no march reported
// yet, that call's backward re-marches).
uint32_t* march_estimate(const SizeKey& key, const Dims& d, bool create, size_t* seq_steps = nullptr) {
    std::lock_guard<std::mutex> lk(g_size_mu);
    SizeGuess& g = g_size_cache[key];
    if (!g.seq_steps && create && !(g.seq_steps = reinterpret_cast<uint32_t*>(pinned_words()))) (void)hipGetLastError();
    if (seq_steps) {
        const uint64_t longest = g.seq_steps ? *reinterpret_cast<volatile uint32_t*>(g.seq_steps) : 0u;
        // (beyond the budget the longest rays do not fit and such a call re-marches)
        *seq_steps = longest ? (size_t)std::min<uint64_t>((longest + longest / 4 + 4 + 3) / 4 * 4, march_budget_steps(d)) : 0;
    }
    return g.seq_steps;
}

using dmr::SizeOut;  // where the kernel that computes a size publishes it: the size port, dmr_kernels.hpp
using dmr::NOWHERE;

// One speculatively sized buffer: its estimate, its largest size (the clamp of a guess; an exact size above it is the error
// too_large), its word in SizeRead, the error of an asynchronous call without an estimate.
struct Sizing { double SizeGuess::* estimate; uint64_t limit; int word; const char* too_large; const char* no_estimate; };

// The speculative sizing above, for both buffers.  first(guess, out): the stages that can be enqueued before the size is
// known, `guess` the capacity (0: no estimate), `out` where the size goes; then(size, redo): the stages that need the exact
// size (redo: they ran with a guess too small).  *size: the exact size, or an asynchronous call's capacity.
// placed_capacity (0: none): the capacity of a placement (above), which takes the estimate's place as the guess; what then decides the
// redo is not the size but the SIZE_WORD_OVERFLOW bit of the size word -- a tile outgrew its segment.
template <class First, class Then>
int sized(const Sizing& z, const SizeKey& key, size_t BF, bool async, hipStream_t st, uint64_t placed_capacity, uint64_t* size, First first, Then then) {
    int dev = 0;
    DMR_HIP(hipGetDevice(&dev));
    uint32_t* overflow = overflow_word(dev, !async);
    uint64_t guess = placed_capacity;
    if (!placed_capacity) {
        std::lock_guard<std::mutex> lk(g_size_mu);
        const double per_face = lookup_estimate(key, z.estimate);
        if (per_face > 0.0) guess = std::min<uint64_t>(padded((uint64_t)(per_face * (double)BF)), z.limit);
    }
    if (async) {  // no host wait at all: capacity from the estimate, overflow checked on the device
        if (!guess || !overflow) return fail(z.no_estimate);
        if (first(guess, SizeOut{nullptr, overflow, 0u, (uint32_t)guess})) return 1;
        *size = guess;  // an upper bound the backward accepts in R's place
        DMR_HIP(hipGetLastError());
        return 0;
    }
    SizeRead& sr = g_size_read[dev];
    if (!sr.slot && !(sr.slot = pinned_words())) return fail("hipHostMalloc failed");
    const uint32_t seq = sr.next_seq();
    if (first(guess, SizeOut{const_cast<unsigned long long*>(sr.word(z.word)), nullptr, seq, 0xffffffffu})) return 1;
    unsigned long long n = 0;
    if (wait_size(sr.word(z.word), seq, st, &n)) return 1;  // the call's one host wait (rasterizer_impl.cu:287-292)
    const bool full = placed_capacity ? (n & dmr::SIZE_WORD_OVERFLOW) != 0 : n > guess;
    if (placed_capacity) n &= dmr::SIZE_WORD_OVERFLOW - 1ull;
    if (n > z.limit) return fail(z.too_large);
    *size = n;
    if (!guess) {
        if (then(n, false)) return 1;
    } else if (full) {  // the guess was too small (a segment, with a placement): redo the affected stages with the exact size
        g_redo_count.fetch_add(1, std::memory_order_relaxed);
        DMR_HIP(hipStreamSynchronize(st));
        if (then(n, true)) return 1;
    }
    {
        std::lock_guard<std::mutex> lk(g_size_mu);
        g_size_cache[key].*z.estimate = (double)std::max<uint64_t>(n, 1) / (double)std::max<size_t>(BF, 1);
    }
    DMR_HIP(hipGetLastError());
    return 0;
}

// Stages shared by both renderers up to the sorted per-tile lists, then `render` (the renderer's own kernels, which only need
// the scratch buffers, the binning buffer included).  min_seq_steps (tet, a multiple of 4): steps per pixel the march sequence
// has room for whatever the estimate says (DMR_FLAG_TET_FRAGMENTS reads the first K steps of every pixel out of it).
int run_forward(const dmr_scene* s, bool tet, const Dims& d, dmr_alloc_fn alloc, void* ctx, hipStream_t st, int* num_rendered,
                const std::function<void(const Scratch&, dmr::ListSize)>& render, size_t min_seq_steps = 0) {
    const Scratch need = carve_scratch(s, tet, d, nullptr, nullptr, nullptr);
    void* pb = alloc(ctx, DMR_BUF_POINT, need.point_bytes);
    void* fb = alloc(ctx, DMR_BUF_FACE, need.face_bytes);
    void* ib = alloc(ctx, DMR_BUF_IMAGE, need.image_bytes);
    if (!pb || !fb || !ib) return fail("scratch allocation failed");
    Scratch c = carve_scratch(s, tet, d, pb, fb, ib);
    const bool async = is_async(s, st);
    const SizeKey key = size_key(s, tet, d);
    size_t seq_steps = 0;
    if (tet) march_estimate(key, d, !async, &seq_steps);
    seq_steps = std::max(seq_steps, min_seq_steps);
    const bool placed = placement_eligible(tet, d);
    const Placement pl = placed ? find_placement(key, d) : Placement{};

    auto front = [&](SizeOut out) {
        dmr::launch_project_verts(*s, d, c, dmr::NO_SEGMENTS, st);
        dmr::launch_setup_faces(*s, d, c, tet, st);
        dmr::launch_scan_tiles(d, c, out, st);
    };
    // the call's binning buffer, carved into c.bs (none at all: a call with no entries and no march sequence)
    auto binning = [&](uint64_t capacity) -> int {
        BinningState tb;
        const size_t mask_tiles = tet ? 0 : (size_t)d.ntiles;
        void* bb = alloc(ctx, DMR_BUF_BINNING, carve_binning(nullptr, (size_t)capacity, mask_tiles, (size_t)d.ntiles, seq_steps, tb));
        if (!bb && (capacity > 0 || seq_steps > 0)) return fail("binning allocation failed");
        carve_binning(bb, (size_t)capacity, mask_tiles, (size_t)d.ntiles, seq_steps, c.bs);
        return 0;
    };
    bool exact = false;  // the lists come from the exact path: its counts and order are what a placement is built from
    auto rest = [&](uint64_t capacity) -> int {
        if (binning(capacity)) return 1;
        exact = true;
        if (capacity > 0) {
            dmr::launch_scatter_faces(*s, d, c, !tet, st);
            if (!dmr::sorts_own_tiles(d)) dmr::launch_sort_tiles(d, c, st);
        }
        render(c, dmr::NO_LIST_SIZE);
        return 0;
    };
    // speculative placement: projection -> one binning kernel -> render, whose first workgroup leaves the size word
    auto binned = [&](SizeOut out) -> int {
        if (binning(pl.capacity)) return 1;
        dmr::launch_project_verts(*s, d, c, dmr::SegInit{pl.start, pl.order}, st);
        dmr::launch_bin_faces(*s, d, c, st);
        render(c, dmr::ListSize{c.is.num_rendered, out, 1u});  // (its first workgroup publishes R)
        return 0;
    };

    const Sizing list_entries{&SizeGuess::rendered_per_face, 0x7fffffffu, 0, "num_rendered overflows 31 bits",
                              "asynchronous / captured call without a size estimate: run one default (waiting) call with the same "
                              "view configuration first"};
    uint64_t R = 0;
    // a redo enqueues the front again too: the scatter pass has used up the tile cursors (a placed call's redo -- a tile outgrew
    // its segment -- goes through the exact path as well)
    int rc = sized(list_entries, key, d.BF, async, st, pl.valid ? pl.capacity : 0, &R,
                   [&](uint64_t guess, SizeOut out) {
                       if (pl.valid) return binned(out);  // (guess = pl.capacity)
                       front(out);
                       return guess ? rest(guess) : 0;
                   },
                   [&](uint64_t size, bool redo) { if (redo) front(NOWHERE); return rest(size); });
    *num_rendered = (int)R;
    if (rc == 0 && placed && !async) {  // the exact path refreshes the placement; one twice as large as the scene needs is dropped
        if (exact) rc = build_placement(key, d, R, c.is, st);
        else if (2 * R < pl.built_from) drop_placement(key);
    }
    return rc;
}

// ---- per-stage timing ---------------------------------------------------------------------------
std::atomic<uint32_t> g_prof_mask{0};
struct ProfRec { int stage; hipEvent_t a, b; };
std::mutex g_prof_mu;
std::vector<ProfRec*> g_prof_live, g_prof_free;

}  // namespace

namespace dmr {
StageScope::StageScope(int stage_, hipStream_t st_) : stage(stage_), st(st_), rec(nullptr) {
    if (!(g_prof_mask.load(std::memory_order_relaxed) & (1u << stage))) return;
    ProfRec* r = nullptr;
    {
        std::lock_guard<std::mutex> lk(g_prof_mu);
        if (!g_prof_free.empty()) { r = g_prof_free.back(); g_prof_free.pop_back(); }
    }
    if (!r) {
        r = new ProfRec();
        if (hipEventCreate(&r->a) != hipSuccess || hipEventCreate(&r->b) != hipSuccess) { delete r; return; }
    }
    r->stage = stage;
    (void)hipEventRecord(r->a, st);
    rec = r;
}
StageScope::~StageScope() {
    if (!rec) return;
    ProfRec* r = reinterpret_cast<ProfRec*>(rec);
    (void)hipEventRecord(r->b, st);
    std::lock_guard<std::mutex> lk(g_prof_mu);
    g_prof_live.push_back(r);
}
// dmr_last_error()'s message, for a translation unit with exports of its own (dmr_shade.hip); returns 1
int api_fail(const char* m) { return fail(m); }
}  // namespace dmr

extern "C" {

void dmr_profile_enable(uint32_t mask) { g_prof_mask.store(mask); }

int dmr_profile_collect(double* ms, int64_t* launches) {
    std::vector<ProfRec*> live;
    {
        std::lock_guard<std::mutex> lk(g_prof_mu);
        live.swap(g_prof_live);
    }
    int rc = 0;
    for (ProfRec* r : live) {
        float t = 0.f;
        if (hipEventSynchronize(r->b) != hipSuccess || hipEventElapsedTime(&t, r->a, r->b) != hipSuccess) {
            g_err = "profile event read failed";
            rc = 1;
        } else if (r->stage >= 0 && r->stage < DMR_NUM_STAGES) {
            if (ms) ms[r->stage] += (double)t;
            if (launches) launches[r->stage] += 1;
        }
    }
    std::lock_guard<std::mutex> lk(g_prof_mu);
    for (ProfRec* r : live) g_prof_free.push_back(r);
    return rc;
}

const char* dmr_stage_name(int stage) {
    static const char* names[DMR_NUM_STAGES] = {"k_project_verts", "k_setup_faces", "k_scan_tiles", "k_scatter_faces",
                                                "k_sort_tiles", "k_tri_forward", "k_tri_backward_pix", "k_tri_unpack",
                                                "k_tet_first_intersect", "k_tet_forward", "k_tet_backward",
                                                "k_tri_backward_hits"};
    return (stage >= 0 && stage < DMR_NUM_STAGES) ? names[stage] : "?";
}

const char* dmr_last_error(void) { return g_err.c_str(); }

int dmr_overflowed(int device, int reset) {
    int dev = device;
    if (dev < 0 && hipGetDevice(&dev) != hipSuccess) return 0;
    uint32_t* w = overflow_word(dev, false);
    if (!w) return 0;
    volatile uint32_t* v = w;
    const int r = *v != 0u;
    if (reset) *v = 0u;
    return r;
}
uint64_t dmr_redo_count(void) { return g_redo_count.load(std::memory_order_relaxed); }
int dmr_abi_version(void) { return DMR_ABI_VERSION; }
const char* dmr_build_arch(void) { return "gfx950"; }

int dmr_tri_forward(const dmr_scene* s, float* out_color, float* out_depth, dmr_alloc_fn alloc, void* ctx,
                    void* stream, int* num_rendered) {
    Dims d;
    if (check_scene(s, false, d)) return 1;
    if (!alloc || !num_rendered || !out_color || !out_depth) return fail("null argument");
    *num_rendered = 0;
    // DMR_FLAG_TRI_FRAGMENTS: K fragment slots per pixel, K in bits 8-15 of the flags
    const int frag_k = fragment_k(s, DMR_FLAG_TRI_FRAGMENTS, "DMR_FLAG_TRI_FRAGMENTS", "DMR_FRAGMENTS_FLAGS(K)");
    if (frag_k < 0) return 1;
    if (s->P == 0 || s->F == 0) return 0;  // render.cu:105 (and Q16: F == 0)
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    float* fragments = nullptr;  // the caller's [face | bary | count], requested once
    if (caller_output(alloc, ctx, DMR_BUF_TRI_FRAGMENTS, frag_k ? dmr::FragmentLists::bytes(d.npix, frag_k) : 0, "tri fragment", false, st, &fragments))
        return 1;
    Scratch last{};  // the scratch of the call's final k_tri_forward: a redo (a refuted size estimate) renders a second time
    auto render = [&](const Scratch& c, dmr::ListSize size) {
        dmr::launch_tri_forward(canonical(s, c.is.mats), d, c, out_color, out_depth, (s->flags & DMR_FLAG_ALPHA) != 0, size, st);
        last = c;
    };
    if (run_forward(s, false, d, alloc, ctx, st, num_rendered, render)) return 1;
    // the fragments describe the colour the call returns: one launch, behind whichever k_tri_forward was the last
    if (fragments && last.is.n_contrib) {
        dmr::launch_tri_fragments(canonical(s, last.is.mats), d, last, frag_k, fragments, st);
        DMR_HIP(hipGetLastError());
    }
    return 0;
}

int dmr_tri_backward(const dmr_scene* s, const float* dL_dcolor, const float* dL_ddepth, int num_rendered,
                     const void* point_buf, const void* face_buf, const void* binning_buf, const void* image_buf,
                     float* dL_dverts, float* dL_dvcolor, float* dL_dfopacity, float* dL_dvdepth, float* dL_dfintense,
                     dmr_alloc_fn alloc, void* ctx, void* stream) {
    Dims d;
    if (check_scene(s, false, d)) return 1;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    // DMR_FLAG_TRI_FRAGMENT_GRADS: K slots per pixel in bits 8-15 of the flags, as for the forward
    const int frag_k = fragment_k(s, DMR_FLAG_TRI_FRAGMENT_GRADS, "DMR_FLAG_TRI_FRAGMENT_GRADS", "DMR_FRAGMENTS_K");
    if (frag_k < 0) return 1;
    // DMR_FLAG_TRI_EXACT_GRADS / DMR_FLAG_TRI_CAMERA_GRADS: which k_tri_backward_hits; with camera gradients the caller's
    // [B][dL/dinv_mv 16 | dL/dinv_proj 16] buffer, requested once
    const bool camera = (s->flags & DMR_FLAG_TRI_CAMERA_GRADS) != 0;
    const int grads = camera ? dmr::TRI_GRAD_CAMERA : ((s->flags & DMR_FLAG_TRI_EXACT_GRADS) ? dmr::TRI_GRAD_EXACT : dmr::TRI_GRAD_REF);
    // Nothing to back-propagate: no geometry (render.cu:173), nothing on screen, or an empty tile-row band (a rank without
    // rows; the asynchronous forward of such a band returns its capacity as num_rendered, hence the band test of its own).
    const bool idle = s->P == 0 || s->F == 0 || num_rendered <= 0 || d.r1 <= d.r0;
    float* cam_out = nullptr;
    if (caller_output(alloc, ctx, DMR_BUF_TRI_CAMERA_GRADS, camera ? 128 * (size_t)s->B : 0, "tri camera gradient", idle, st, &cam_out)) return 1;
    // the caller's two inputs, requested once each (not when idle: the term is zero then)
    const int32_t* frag_face = nullptr;
    const float* frag_grad = nullptr;
    if (frag_k && !idle && fragment_grad_inputs(alloc, ctx, "tri", "TRI", DMR_BUF_TRI_FRAGMENT_FACES, DMR_BUF_TRI_FRAGMENT_BARY_GRADS, d.npix, frag_k, &frag_face, &frag_grad))
        return 1;
    if (idle) {
        if (s->P > 0) {
            DMR_HIP(hipMemsetAsync(dL_dverts, 0, sizeof(float) * 3 * (size_t)s->P, st));
            DMR_HIP(hipMemsetAsync(dL_dvcolor, 0, sizeof(float) * 3 * (size_t)s->P, st));
            DMR_HIP(hipMemsetAsync(dL_dvdepth, 0, sizeof(float) * d.BP, st));
        }
        if (s->F > 0) {
            DMR_HIP(hipMemsetAsync(dL_dfopacity, 0, sizeof(float) * (size_t)s->F, st));
            DMR_HIP(hipMemsetAsync(dL_dfintense, 0, sizeof(float) * d.BF, st));
        }
        if (s->P > 0 && s->F > 0) {  // a default call leaves an estimate behind even so: later asynchronous calls need one
            std::lock_guard<std::mutex> lk(g_size_mu);
            SizeGuess& g = g_size_cache[size_key(s, false, d)];
            if (!(g.hits_per_face > 0.0)) g.hits_per_face = 1.0 / (double)std::max<size_t>(d.BF, 1);
        }
        return 0;
    }
    if (!point_buf || !face_buf || !binning_buf || !image_buf || !alloc) return fail("null scratch buffer");
    const Scratch c = carve_scratch(s, false, d, point_buf, face_buf, image_buf, binning_buf, (size_t)num_rendered);
    const ImageState& is = c.is;

    // The forward counted the blended (pixel, face) pairs per tile and in total; the total sizes the record
    // buffer (the backward's one 8-byte host read; speculative sizing as in the forward).
    const size_t vbytes = up(sizeof(float) * dmr::VROW * d.BP), fbytes = up(sizeof(float) * dmr::FROW * d.BF);
    const size_t pbytes = up(sizeof(float4) * 2 * (size_t)d.ntiles * dmr::TILE_PIX);  // per tile: its 256 pixels' (ray, upstream gradient) records
    const size_t cbytes = camera ? up(sizeof(float) * 32 * (size_t)d.ntiles) : 0;  // camera gradients: every tile's partial
    // regions: see dmr::HitRegions -- null hit_offset: launch_scan_hits has laid the record regions out
    auto rest = [&](uint64_t capacity, dmr::HitRegions regions) -> int {
        const size_t hbytes = up(sizeof(dmr::HitRecord) * (size_t)capacity);
        char* work = reinterpret_cast<char*>(alloc(ctx, DMR_BUF_WORK, vbytes + fbytes + cbytes + pbytes + hbytes));
        if (!work) return fail("workspace allocation failed");
        float* vrow = reinterpret_cast<float*>(work);
        float* frow = reinterpret_cast<float*>(work + vbytes);
        float* cam_part = reinterpret_cast<float*>(work + vbytes + fbytes);  // (zeroed with the accumulators)
        float4* pixrec = reinterpret_cast<float4*>(work + vbytes + fbytes + cbytes);
        dmr::HitRecord* hits = reinterpret_cast<dmr::HitRecord*>(work + vbytes + fbytes + cbytes + pbytes);
        const dmr_scene sc = canonical(s, is.mats);
        // (Splitting the tiles into bands whose hit-parallel kernel runs on a second stream while the next band's
        // per-pixel kernel computes -- atomic unit and SIMDs busy at the same time -- was measured and lost: 0.56 ms
        // per step with 1 band, 0.64 with 2, 0.70 with 4 at C4; cross-stream event waits cost more than the overlap.)
        // k_tri_backward_pix also zeroes the packed accumulators (every block a slice).  (Handing out the tiles'
        // record regions from an atomic cursor: the 2.9 k returning same-address atomics stall their waves, in order
        // with every younger load -- 17 us.)
        dmr::launch_tri_backward_pix(sc, d, c, dL_dcolor, dL_ddepth, pixrec, hits, (uint32_t)capacity, reinterpret_cast<float*>(work),
                                     (vbytes + fbytes + cbytes) / sizeof(float), regions,
                                     (s->flags & DMR_FLAG_ALPHA) != 0, st);  // (dL_ddepth [B,2,H,W]: its alpha channel reaches dL_dfopacity)
        dmr::launch_tri_backward_hits(sc, d, c, pixrec, hits, (uint32_t)capacity, vrow, frow, grads, camera ? cam_part : nullptr, st);
        // the fragment lists' term joins the packed vertex rows (and the tiles' camera partials) before they are unpacked / reduced
        if (frag_face)
            dmr::launch_tri_fragment_grads(sc, d, c, frag_k, frag_face, frag_grad, vrow, camera ? cam_part : nullptr, st);
        dmr::launch_tri_unpack(*s, vrow, frow, dL_dverts, dL_dvcolor, dL_dfopacity, dL_dvdepth, dL_dfintense, st);
        if (camera) dmr::launch_camera_reduce(s->B, d.gx * d.gy, 32, cam_part, cam_out, st);
        return 0;
    };
    const dmr::HitRegions scanned{nullptr, nullptr, NOWHERE};
    auto self_laid = [&](SizeOut out) { return dmr::HitRegions{is.hit_offset, is.hit_total, out}; };
    // With a size estimate and few enough tiles the per-pixel kernel lays the regions out itself: no scan launch.
    const bool self_regions = d.ntiles <= dmr::SCAN_SINGLE_MAX;
    auto first = [&](uint64_t guess, SizeOut out) -> int {
        if (guess && self_regions) return rest(guess, self_laid(out));
        dmr::launch_scan_hits(d, c, out, st);
        return guess ? rest(guess, scanned) : 0;
    };
    const Sizing hit_records{&SizeGuess::hits_per_face, 0xfffffffeu, 1, "more than 2^32 blended (pixel, face) pairs",
                             "asynchronous / captured call without a size estimate: run one default (waiting) backward with the "
                             "same view configuration first"};
    uint64_t nhits = 0;
    // a redo re-runs the record passes only: the scan's regions still stand
    return sized(hit_records, size_key(s, false, d), d.BF, is_async(s, st), st, 0, &nhits, first,
                 [&](uint64_t exact, bool redo) { return rest(exact, redo && self_regions ? self_laid(NOWHERE) : scanned); });
}

int dmr_tet_forward(const dmr_scene* s, float* out_color, float* out_depth, float* out_active, dmr_alloc_fn alloc,
                    void* ctx, void* stream, int* num_rendered) {
    Dims d;
    if (check_scene(s, true, d)) return 1;
    if (!alloc || !num_rendered || !out_color || !out_depth || !out_active) return fail("null argument");
    *num_rendered = 0;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    // DMR_FLAG_TET_FRAGMENTS: K fragment slots per pixel, K in bits 8-15 of the flags as for the tri flag
    int frag_k = fragment_k(s, DMR_FLAG_TET_FRAGMENTS, "DMR_FLAG_TET_FRAGMENTS", "DMR_TET_FRAGMENTS_FLAGS(K)");
    if (frag_k < 0) return 1;
    if (s->P == 0 || s->F == 0) frag_k = 0;  // nothing marches: the caller's initialisation (-1 / 0) is the result, no request
    // the fragments are read out of the march sequence: room for the first K steps of every pixel, whatever the estimate says
    const size_t frag_steps = ((size_t)frag_k + 3) / 4 * 4;
    if (frag_steps > march_budget_steps(d))
        return fail("DMR_FLAG_TET_FRAGMENTS: K = " + std::to_string(frag_k) + " needs a march sequence of " +
                    std::to_string(dmr::tet_seq_bytes((size_t)d.ntiles, frag_steps)) + " bytes (" + std::to_string(frag_steps) +
                    " steps for each of " + std::to_string((size_t)d.ntiles * dmr::TILE_PIX) + " tile pixels), beyond the budget of " +
                    std::to_string(TET_SEQ_BUDGET) + " bytes (16 GiB)");
    float* fragments = nullptr;  // the caller's [face | bary | count], requested once
    if (caller_output(alloc, ctx, DMR_BUF_TET_FRAGMENTS, frag_k ? dmr::FragmentLists::bytes(d.npix, frag_k) : 0, "tet fragment", false, st, &fragments))
        return 1;
    auto render = [&](const Scratch& c, dmr::ListSize) {
        const dmr_scene sc = canonical(s, c.is.mats);
        dmr::launch_tet_prep(sc, d, c, st);
        dmr::launch_tet_first_intersect(sc, d, c, st);
        dmr::launch_tet_forward(sc, d, c, out_color, out_depth, out_active, (s->flags & DMR_FLAG_ALPHA) != 0, st);
        // the fragments describe the images the call returns: behind every k_tet_forward, so after a redo the redo's
        if (fragments) dmr::launch_tet_fragments(sc, d, c, frag_k, fragments, st);
    };
    return run_forward(s, true, d, alloc, ctx, st, num_rendered, render, frag_steps);
}

int dmr_tet_backward(const dmr_scene* s, const float* dL_dcolor, const float* dL_ddepth, const void* point_buf,
                     const void* face_buf, const void* binning_buf, const void* image_buf, float* dL_dvcolor,
                     float* dL_dfopacity, dmr_alloc_fn alloc, void* ctx, void* stream) {
    Dims d;
    if (check_scene(s, true, d)) return 1;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    // DMR_FLAG_TET_FRAGMENT_GRADS (implies the full gradients): K slots per pixel in bits 8-15 of the flags, as for the forward
    const int frag_k = fragment_k(s, DMR_FLAG_TET_FRAGMENT_GRADS, "DMR_FLAG_TET_FRAGMENT_GRADS", "DMR_FRAGMENTS_K");
    if (frag_k < 0) return 1;
    // DMR_FLAG_TET_CAMERA_GRADS (implies the full gradients): the caller's [B][dL/dinv_mv 16 | dL/dinv_proj 16 | dL/dmv 16 |
    // dL/dproj 16] buffer, requested once, summed from per-tile partials in the work space
    const bool camera = (s->flags & DMR_FLAG_TET_CAMERA_GRADS) != 0;
    // the camera gradients of a call with nothing to back-propagate (no geometry, or an empty tile-row band: a rank without
    // rows) are zeros
    const int band_tiles = d.gx * (d.r1 - d.r0);  // per view
    float* cam_out = nullptr;
    if (caller_output(alloc, ctx, DMR_BUF_TET_CAMERA_GRADS, camera ? 256 * (size_t)s->B : 0, "tet camera gradient",
                      s->P == 0 || s->F == 0 || band_tiles == 0, st, &cam_out))
        return 1;
    float* full = nullptr;  // DMR_FLAG_TET_FULL_GRADS: [dL_dverts 3P | dL_dfintense BF], zeroed by the launch that follows
    const bool full_grads = (s->flags & (DMR_FLAG_TET_FULL_GRADS | DMR_FLAG_TET_CAMERA_GRADS | DMR_FLAG_TET_FRAGMENT_GRADS)) != 0;
    if (caller_output(alloc, ctx, DMR_BUF_TET_GRADS, full_grads ? sizeof(float) * (3 * (size_t)s->P + d.BF) : 0, "tet gradient", false, st, &full))
        return 1;
    if (full) dmr::launch_tet_zero_grads(full, 3 * (int64_t)s->P, full + 3 * (int64_t)s->P, (int64_t)d.BF, st);
    dmr::launch_tet_zero_grads(dL_dvcolor, 3 * (int64_t)s->P, dL_dfopacity, (int64_t)s->F, st);
    if (s->P == 0 || s->F == 0) return 0;
    if (!image_buf || !face_buf) return fail("null scratch buffer");
    // the caller's two inputs, requested once each (not for an empty band: the term is zero then)
    const int32_t* frag_face = nullptr;
    const float* frag_grad = nullptr;
    if (frag_k && band_tiles > 0 && fragment_grad_inputs(alloc, ctx, "tet", "TET", DMR_BUF_TET_FRAGMENT_FACES, DMR_BUF_TET_FRAGMENT_BARY_GRADS, d.npix, frag_k, &frag_face, &frag_grad))
        return 1;
    float* cam_part = nullptr;  // every tile's partial (launch_tet_backward)
    if (cam_out) {
        cam_part = static_cast<float*>(alloc(ctx, DMR_BUF_WORK, 256 * (size_t)band_tiles * (size_t)s->B));
        if (!cam_part) return fail("workspace allocation failed");
    }
    // binning_buf: the forward's march sequence lives there (where and how much of it: is.seq, on the device); a null
    // buffer is fine when the forward ran without one (its descriptor then says cap = 0 and the backward re-marches)
    const Scratch c = carve_scratch(s, true, d, point_buf, face_buf, image_buf, binning_buf);
    const dmr_scene sc = canonical(s, c.is.mats);
    uint32_t* host_seq_steps = march_estimate(size_key(s, true, d), d, false);
    dmr::launch_tet_backward(sc, d, c, dL_dcolor, dL_ddepth, dL_dvcolor, dL_dfopacity, host_seq_steps, full,
                             full ? full + 3 * (int64_t)s->P : nullptr, cam_part, (s->flags & DMR_FLAG_ALPHA) != 0, st);
    // the fragment lists' term joins dL_dverts (and the tiles' camera partials) before the partials are reduced
    if (frag_face) dmr::launch_tet_fragment_grads(sc, d, c, frag_k, frag_face, frag_grad, full, cam_part, st);
    if (cam_out) dmr::launch_camera_reduce(s->B, band_tiles, 64, cam_part, cam_out, st);
    DMR_HIP(hipGetLastError());
    return 0;
}

// ---- 4x4 inverses (caller-side step) ---------------------------------------
namespace {
__global__ void k_invert_mats(const float* __restrict__ in, int count, int transposed, float* __restrict__ out) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= count) return;
    double a[16];
#pragma unroll
    for (int k = 0; k < 16; k++) a[k] = (double)in[16 * m + (transposed ? 4 * (k & 3) + (k >> 2) : k)];  // a[4*i + j]
    // cofactor expansion with the six 2x2 minors of the upper and of the lower two rows
    const double s0 = a[0] * a[5] - a[1] * a[4], s1 = a[0] * a[6] - a[2] * a[4], s2 = a[0] * a[7] - a[3] * a[4];
    const double s3 = a[1] * a[6] - a[2] * a[5], s4 = a[1] * a[7] - a[3] * a[5], s5 = a[2] * a[7] - a[3] * a[6];
    const double c5 = a[10] * a[15] - a[11] * a[14], c4 = a[9] * a[15] - a[11] * a[13], c3 = a[9] * a[14] - a[10] * a[13];
    const double c2 = a[8] * a[15] - a[11] * a[12], c1 = a[8] * a[14] - a[10] * a[12], c0 = a[8] * a[13] - a[9] * a[12];
    const double det = s0 * c5 - s1 * c4 + s2 * c3 + s3 * c2 - s4 * c1 + s5 * c0;
    const double r = 1.0 / det;
    double b[16];
    b[0] = (a[5] * c5 - a[6] * c4 + a[7] * c3) * r;   b[1] = (-a[1] * c5 + a[2] * c4 - a[3] * c3) * r;
    b[2] = (a[13] * s5 - a[14] * s4 + a[15] * s3) * r; b[3] = (-a[9] * s5 + a[10] * s4 - a[11] * s3) * r;
    b[4] = (-a[4] * c5 + a[6] * c2 - a[7] * c1) * r;  b[5] = (a[0] * c5 - a[2] * c2 + a[3] * c1) * r;
    b[6] = (-a[12] * s5 + a[14] * s2 - a[15] * s1) * r; b[7] = (a[8] * s5 - a[10] * s2 + a[11] * s1) * r;
    b[8] = (a[4] * c4 - a[5] * c2 + a[7] * c0) * r;   b[9] = (-a[0] * c4 + a[1] * c2 - a[3] * c0) * r;
    b[10] = (a[12] * s4 - a[13] * s2 + a[15] * s0) * r; b[11] = (-a[8] * s4 + a[9] * s2 - a[11] * s0) * r;
    b[12] = (-a[4] * c3 + a[5] * c1 - a[6] * c0) * r; b[13] = (a[0] * c3 - a[1] * c1 + a[2] * c0) * r;
    b[14] = (-a[12] * s3 + a[13] * s1 - a[14] * s0) * r; b[15] = (a[8] * s3 - a[9] * s1 + a[10] * s0) * r;
#pragma unroll
    for (int k = 0; k < 16; k++) out[16 * m + k] = (float)b[k];
}
}  // namespace

int dmr_invert_mats(const float* in, int count, int transposed, float* out, void* stream) {
    if (count < 0 || (count > 0 && (!in || !out))) return fail("dmr_invert_mats: bad arguments");
    if (count == 0) return 0;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    k_invert_mats<<<dim3((unsigned)((count + 63) / 64)), dim3(64), 0, st>>>(in, count, transposed, out);
    DMR_HIP(hipGetLastError());
    return 0;
}

// ---- parity/debug export ---------------------------------------------------------------------
namespace {
__global__ void k_export_vproj(const float4* v, int64_t n, int what, float* dst) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (what == 0) { dst[2 * i] = v[i].x; dst[2 * i + 1] = v[i].y; }
    else dst[i] = v[i].z;
}
__global__ void k_export_ranges(const uint32_t* off, const uint32_t* cnt, int64_t n, uint32_t* dst) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    // the reference leaves empty tiles at (0, 0) (cudaMemset, rasterizer_impl.cu:330)
    const bool empty = cnt[i] == 0;
    dst[2 * i] = empty ? 0u : off[i];
    dst[2 * i + 1] = empty ? 0u : off[i + 1];
}
}  // namespace

int64_t dmr_export(const dmr_scene* s, int is_tet, int num_rendered, const char* name, const void* point_buf,
                   const void* face_buf, const void* binning_buf, const void* image_buf, void* dst, int64_t cap,
                   void* stream) {
    Dims d;
    if (!name || check_scene(s, is_tet != 0, d)) return -1;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const Scratch c = carve_scratch(s, is_tet != 0, d, point_buf, face_buf, image_buf, binning_buf, (size_t)std::max(0, num_rendered));
    const FaceState& fs = c.fs; const ImageState& is = c.is;
    const std::string n(name);
    auto plain = [&](const void* src, size_t bytes) -> int64_t {
        if (dst && src && bytes) {
            if (hipMemcpyAsync(dst, src, std::min<size_t>(bytes, (size_t)cap), hipMemcpyDeviceToDevice, st) != hipSuccess) {
                g_err = "export copy failed";
                return -1;
            }
        }
        return (int64_t)bytes;
    };
    if (n == "image" || n == "ndc_z") {
        const size_t bytes = d.BP * (n == "image" ? 8 : 4);
        if (dst && d.BP && (size_t)cap >= bytes)
            k_export_vproj<<<dim3((unsigned)((d.BP + 255) / 256)), dim3(256), 0, st>>>(
                c.ps.vproj, (int64_t)d.BP, n == "image" ? 0 : 1, reinterpret_cast<float*>(dst));
        return (int64_t)bytes;
    }
    // Tri lists up to SCAN_SINGLE_MAX tiles may lie in padded segments (speculative placement): [tile_offset, list end).  The
    // exports stay what the exact path's are -- contiguous ranges, packed face_list -- compacted here on the host (a waiting,
    // untimed debug path either way).
    if (!is_tet && d.ntiles <= dmr::SCAN_SINGLE_MAX && (n == "ranges" || n == "face_list")) {
        const size_t nt = (size_t)d.ntiles, R = (size_t)std::max(0, num_rendered);
        const size_t bytes = n == "ranges" ? nt * 8 : R * 4;
        if (!dst || (size_t)cap < bytes || bytes == 0) return (int64_t)bytes;
        if (!image_buf || (n == "face_list" && !binning_buf)) { g_err = "null scratch buffer"; return -1; }
        std::vector<uint32_t> off(nt + 1), end(nt), out(bytes / 4, 0u);
        if (hipStreamSynchronize(st) != hipSuccess || hipMemcpy(off.data(), is.tile_offset, 4 * (nt + 1), hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(end.data(), is.tile_cursor, 4 * nt, hipMemcpyDeviceToHost) != hipSuccess) { g_err = "export copy failed"; return -1; }
        std::vector<uint32_t> lists;
        if (n == "face_list") {
            lists.resize(off[nt]);
            if (off[nt] && hipMemcpy(lists.data(), c.bs.face_list, 4 * (size_t)off[nt], hipMemcpyDeviceToHost) != hipSuccess) { g_err = "export copy failed"; return -1; }
        }
        size_t run = 0;
        for (size_t t = 0; t < nt; t++) {
            const size_t len = dmr::list_end(off.data(), end.data(), (int)t) - off[t];
            if (n == "ranges") { out[2 * t] = len ? (uint32_t)run : 0u; out[2 * t + 1] = len ? (uint32_t)(run + len) : 0u; }
            else for (size_t k = 0; k < len && run + k < R; k++) out[run + k] = lists[off[t] + k];
            run += len;
        }
        if (hipMemcpy(dst, out.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) { g_err = "export copy failed"; return -1; }
        return (int64_t)bytes;
    }
    if (n == "ranges") {
        const size_t bytes = (size_t)d.ntiles * 8;
        if (dst && (size_t)cap >= bytes)
            k_export_ranges<<<dim3((unsigned)((d.ntiles + 255) / 256)), dim3(256), 0, st>>>(
                is.tile_offset, is.tile_count, d.ntiles, reinterpret_cast<uint32_t*>(dst));
        return (int64_t)bytes;
    }
    if (n == "key_depth") return plain(fs.key_depth, d.BF * 4);
    if (n == "max_depth") return is_tet ? plain(fs.max_depth, d.BF * 4) : -1;
    if (n == "tiles_touched") return plain(fs.tiles_touched, d.BF * 4);
    if (n == "face_list") return plain(c.bs.face_list, (size_t)std::max(0, num_rendered) * 4);
    if (n == "final_T") return plain(is.final_T, d.npix * 4);
    if (n == "final_prev_T") return plain(is.final_prev_T, d.npix * 4);
    if (n == "n_contrib") return plain(is.n_contrib, d.npix * 4);
    if (n == "tile_hits") return is_tet ? -1 : plain(is.tile_hits, (size_t)d.ntiles * 4);
    if (is_tet) {
        if (n == "first_face") return plain(is.first_face, d.npix * 4);
        if (n == "first_tet") return plain(is.first_tet, d.npix * 4);
        if (n == "last_face") return plain(is.last_face, d.npix * 4);
        if (n == "last_tet") return plain(is.last_tet, d.npix * 4);
        if (n == "is_active") return plain(is.is_active, d.npix);
        if (n == "tet_seq") return plain(is.seq, 8);  // {longest march, steps the forward's march sequence had room for}
    }
    g_err = "unknown export item: " + n;
    return -1;
}

}  // extern "C"
