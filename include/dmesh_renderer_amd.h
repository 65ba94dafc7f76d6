/*
 * dmesh_renderer_amd.h -- C ABI of libdmesh_renderer_hip.so (MI355X / gfx950).
 *
 * This is the drop-in boundary for the hot path of SonSang/dmesh_renderer: the four
 * entry points below replace what the reference's pybind module `_C` (ext.cpp:6-11)
 * reaches through render.cu:
 *
 *   dmr_tri_forward   <- CudaRasterizer::Rasterizer::forward  (cuda_rasterizer/rasterizer.h:13-42,
 *                        called from RasterizeTrianglesCUDA, render.cu:107-129)
 *   dmr_tri_backward  <- CudaRasterizer::Rasterizer::backward (rasterizer.h:44-67, render.cu:175-204)
 *   dmr_tet_forward   <- CudaRenderer::Renderer::forward      (cuda_renderer/renderer.h:12-46, render.cu:303-334)
 *   dmr_tet_backward  <- CudaRenderer::Renderer::backward     (renderer.h:48-75, render.cu:378-409)
 *
 * Plain pointers and sizes only: every pointer is a DEVICE pointer unless stated,
 * tensors are dense row-major fp32 / int32 exactly as render.cu hands them down
 * (`.contiguous().data<T>()`), matrices are [B,16] column-major m[4*col+row]
 * (auxiliary.h:71-90) unless dmr_scene.mats_transposed says otherwise.  `stream` is a hipStream_t (NULL = default stream).  All work
 * is enqueued on that stream; the only host synchronisation is the wait for the 4-byte num_rendered in the forward
 * calls and for the 8-byte record count in the tri backward (reference: rasterizer_impl.cu:287-292), and not even that
 * with DMR_FLAG_ASYNC or under stream capture ("Sizes only the device knows" below).
 *
 * Return value: 0 on success, non-zero on error; dmr_last_error() then returns a
 * message for the calling thread (the glue raises RuntimeError with it, as the
 * reference's CHECK_CUDA -> std::runtime_error does, auxiliary.h:425-432).
 */
#ifndef DMESH_RENDERER_AMD_H
#define DMESH_RENDERER_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DMR_ABI_VERSION 4

/* Scratch buffers.  The first four are the reference's pointBuffer / faceBuffer /
 * binningBuffer / imageBuffer (rasterizer.h:14-17): opaque byte buffers that the
 * caller owns, returns from forward and passes back to backward.  DMR_BUF_WORK is a
 * transient workspace of the backward calls (packed gradient accumulators). */
enum { DMR_BUF_POINT = 0, DMR_BUF_FACE = 1, DMR_BUF_BINNING = 2, DMR_BUF_IMAGE = 3, DMR_BUF_WORK = 4,
       DMR_BUF_TET_GRADS = 5 /* dmr_tet_backward with DMR_FLAG_TET_FULL_GRADS: an OUTPUT, see there */,
       DMR_BUF_TRI_CAMERA_GRADS = 6 /* dmr_tri_backward with DMR_FLAG_TRI_CAMERA_GRADS: an OUTPUT, see there */,
       DMR_BUF_TET_CAMERA_GRADS = 7 /* dmr_tet_backward with DMR_FLAG_TET_CAMERA_GRADS: an OUTPUT, see there */,
       DMR_BUF_TRI_FRAGMENTS = 8 /* dmr_tri_forward with DMR_FLAG_TRI_FRAGMENTS: an OUTPUT, see the flag */,
       DMR_BUF_TRI_FRAGMENT_FACES = 9 /* dmr_tri_backward with DMR_FLAG_TRI_FRAGMENT_GRADS: an INPUT, see the flag */,
       DMR_BUF_TRI_FRAGMENT_BARY_GRADS = 10 /* dmr_tri_backward with DMR_FLAG_TRI_FRAGMENT_GRADS: an INPUT, see the flag */,
       DMR_BUF_TET_FRAGMENTS = 11 /* dmr_tet_forward with DMR_FLAG_TET_FRAGMENTS: an OUTPUT, see the flag */,
       DMR_BUF_TET_FRAGMENT_FACES = 12 /* dmr_tet_backward with DMR_FLAG_TET_FRAGMENT_GRADS: an INPUT, see the flag */,
       DMR_BUF_TET_FRAGMENT_BARY_GRADS = 13 /* dmr_tet_backward with DMR_FLAG_TET_FRAGMENT_GRADS: an INPUT, see the flag */ };

/* Footprints (bytes; B views, P verts, F faces, T tets, Nt = B * ceil(W/16) * ceil(H/16) tiles, R list entries; every
 * sub-array rounded up to 256): point 16 BP; face 16 BF (tet: 20 BF + 128 F + 224 T); image ~76 B + 40 Nt + 12 BWH (tet: 29 BWH);
 * binning 12 R', R' = R or, with a size estimate, 1.25 R_prev + 4096, or (tri, Nt <= 8192, from the second call of a view
 * configuration on: every tile's list lies in a segment placed from the previous counts) 1.25 R_prev + 32 Nt -- plus, tri only, the coverage masks the forward
 * leaves for the backward: 4096 (R'/128 + min(Nt, R') + 1), i.e. 32 B per list entry and 4 KB per tile that can be busy (a
 * tile's first chunk has the slot of the tile's rank among the busy tiles, so a sparse frame of 1 M tiles pays for its list
 * entries, not 4 GiB for its tiles; the reference's binning buffer scales with R only) -- plus, tet only, the forward's march sequence for
 * the backward: 4 bytes per tile pixel (256 Nt of them) and step of capacity, capacity = the longest march of the previous
 * call with the same view configuration * 1.25 + 4 steps (0 in the first such call), the whole capped at 16 GiB -- with
 * DMR_FLAG_TET_FRAGMENTS at least K rounded up to a multiple of 4 steps, so such a call owns a larger binning buffer than one
 * without the flag only while 1.25 * longest + 4 < K (always in the first call of a view configuration); a K whose steps alone
 * exceed the 16 GiB (about 134 M tile pixels at K = 32) is an error;
 * work (tri backward) 32 BP + 8 BF + 8192 Nt + 16 per hit record (+ 128 Nt with DMR_FLAG_TRI_CAMERA_GRADS); tri camera grads
 * (tri backward with DMR_FLAG_TRI_CAMERA_GRADS only) 128 B, exactly; tet grads (tet backward with DMR_FLAG_TET_FULL_GRADS or
 * DMR_FLAG_TET_CAMERA_GRADS only) 4 (3P + BF), exactly; work (tet backward with DMR_FLAG_TET_CAMERA_GRADS only) 256 per tile of
 * the call's band; tet camera grads (tet backward with DMR_FLAG_TET_CAMERA_GRADS only) 256 B, exactly; tri fragments (tri
 * forward with DMR_FLAG_TRI_FRAGMENTS only) 4 BWH (3K + 1), exactly; tri fragment faces and tri fragment bary grads (tri
 * backward with DMR_FLAG_TRI_FRAGMENT_GRADS only; inputs) 4 BKWH and 8 BKWH, exactly; tet fragments (tet forward with
 * DMR_FLAG_TET_FRAGMENTS only) 4 BWH (3K + 1), exactly; tet fragment faces and tet fragment bary grads (tet backward with
 * DMR_FLAG_TET_FRAGMENT_GRADS only; inputs) 4 BKWH and 8 BKWH, exactly -- that flag implies DMR_FLAG_TET_FULL_GRADS, so such a
 * call also owns the tet grads buffer. */

/* C equivalent of the reference's four std::function<char*(size_t)> allocators
 * (rasterizer.h:14-17, render.cu:18-24): must return a device pointer to at least
 * `nbytes` bytes (256-byte aligned), or NULL on failure.  Called from the calling thread,
 * normally once per buffer per call; a second request for the same buffer replaces the
 * first one -- it happens when a size guess taken from the previous call turned out too small.  The second request is then
 * the larger one, except in a tri forward whose tile segments were placed from the previous counts: there one tile that
 * outgrew its segment is enough, and the exact size then requested may be smaller than the placement's capacity. */
typedef void* (*dmr_alloc_fn)(void* ctx, int which, size_t nbytes);

typedef struct dmr_scene {
    int32_t B, P, F, T, W, H;    /* views, verts, faces, tets (0 for tri), image size */
    const float* background;     /* [3] */
    const float* verts;          /* [P,3] */
    const int32_t* faces;        /* [F,3] */
    const float* verts_color;    /* [P,3] */
    const float* faces_opacity;  /* [F] */
    const float* mv_mats;        /* [B,16] column-major */
    const float* proj_mats;      /* [B,16] */
    const float* inv_mv_mats;    /* [B,16] */
    const float* inv_proj_mats;  /* [B,16] */
    const float* verts_depth;    /* [B,P] */
    const float* faces_intense;  /* [B,F] */
    const int32_t* tets;         /* [T,4]  tet renderer only */
    const int32_t* face_tets;    /* [F,2]  tet renderer only, -1 = no tet */
    const int32_t* tet_faces;    /* [T,4]  tet renderer only */
    int32_t ray_random_seed;     /* tet renderer only; <= 0: rays through pixel centres; > 0: jittered rays, pixel - 0.5 + 0.5 u
                                  * (cuda_renderer/forward.cu:120-123) with u from Philox-4x32-10(key = seed, counter = pixel):
                                  * same distribution as the reference, not its cuRAND XORWOW bits (parity unpinned) */
    /* Tile-row band [row_begin, row_end) this call renders (multi-GPU shard by tile
     * rows); 0,0 means all rows.  Pixels outside the band are left untouched. */
    int32_t row_begin, row_end;
    /* Bit i set (0 mv, 1 proj, 2 inv_mv, 3 inv_proj): matrix i is handed over with its 4x4 blocks transposed,
     * i.e. element k of the [B,16] contract above lives at 16*b + 4*(k & 3) + (k >> 2).  That is the storage
     * behind the `.transpose(1, 2)` views the reference wrapper passes (dmesh_renderer/__init__.py:219-220)
     * and behind th.inverse of such a view, so the glue need not launch the four `.contiguous()` copies of
     * render.cu:117-120.  The forward stores the matrices in contract layout in the image buffer; the
     * backward reads them from there (its matrix arguments are not dereferenced). */
    int32_t mats_transposed;
    /* DMR_FLAG_* bits.  DMR_FLAG_ASYNC: the call never waits for the device (see "Sizes only the device knows"). */
    int32_t flags;
} dmr_scene;

/* Sizes only the device knows.  R (the binning buffer's entries, `num_rendered`) and the number of blended (pixel,
 * face) pairs (the tri backward's record buffer) are results of kernels.  The reference stalls on a device->host copy of
 * R before it can go on (rasterizer_impl.cu:287-299).  Here a call sizes both buffers from the previous call with the
 * same view configuration (+25 %), enqueues everything, and
 *   - by default waits for the size to arrive in pinned host memory (the kernel that computes it stores it there; the host
 *     polls the word: no event, no stream synchronisation, the GPU keeps running), returns the exact R and redoes the
 *     affected stages if the estimate was too small;
 *   - with DMR_FLAG_ASYNC, or when `stream` is being captured into a HIP graph (hipStreamIsCapturing), does not wait at
 *     all: *num_rendered receives the CAPACITY it used (an upper bound that the backward accepts in R's place), every
 *     kernel clamps to it, and a scene that outgrew it sets a sticky per-device flag that dmr_overflowed() reports --
 *     the results of such a call are incomplete (tiles beyond the capacity render as empty) and the caller repeats the
 *     step with a default (waiting) call, which refreshes the estimate.  Needs one earlier default call with the same
 *     view configuration (the warm-up before a capture), else it fails. */
#define DMR_FLAG_ASYNC 1
/* dmr_tet_backward also computes dL/dverts and dL/dfaces_intense (beyond the reference, whose tet renderer has no such
 * gradients); see dmr_tet_backward.  Ignored by every other call. */
#define DMR_FLAG_TET_FULL_GRADS 2
/* dmr_tri_backward writes the exact derivative of the image into dL_dverts instead of the reference's (whose "dv/dp" is
 * dt/dp); see dmr_tri_backward.  Ignored by every other call. */
#define DMR_FLAG_TRI_EXACT_GRADS 4
/* dmr_tri_backward also computes the gradients of the inverse matrices (implies DMR_FLAG_TRI_EXACT_GRADS); see there.
 * Ignored by every other call. */
#define DMR_FLAG_TRI_CAMERA_GRADS 8
/* dmr_tet_backward also computes the gradients of the four matrices (implies DMR_FLAG_TET_FULL_GRADS); see there.
 * Ignored by every other call. */
#define DMR_FLAG_TET_CAMERA_GRADS 16
/* All four calls: the depth image has a second channel, the accumulated opacity (coverage) alpha = 1 - T_final, T_final the
 * transmittance the call multiplies into the background (color == C + (1 - alpha) * background per pixel).  out_depth and
 * dL_ddepth are then [B,2,H,W]: channel 0 the depth as without the flag, channel 1 alpha / its upstream gradient.  alpha is 0
 * where nothing was blended, where a tet pixel's march fails (out_active == 0) and, like the other images, untouched outside
 * the rendered tile rows (the caller zero-initialises).  d alpha / d opacity_i = T_final / (1 - opacity_i) for every blended
 * face i of the pixel (prev_T_final for a face of opacity 1, as for the background terms); alpha depends on nothing else, so
 * the upstream gradient reaches dL_dfopacity only, whatever other gradient flags are set.  No new buffer, no host wait
 * (DMR_FLAG_ASYNC and stream capture work as before); colour and depth are bit for bit those of a call without the flag.
 * Forward and backward of a step must agree on the flag only in the shapes they pass: the scratch buffers are the same. */
#define DMR_FLAG_ALPHA 32
/* dmr_tri_forward only (ignored by every other call): per-pixel fragment lists, what a general rasteriser returns for
 * shading outside it.  K, the slots per pixel, travels in bits 8-15 of the flags: flags |= DMR_FRAGMENTS_FLAGS(K), K in
 * 1..32 (the flag with K = 0 or K > 32 is an error).  The call then requests buffer DMR_BUF_TRI_FRAGMENTS through `alloc`,
 * once, of exactly 4 BWH (3K + 1) bytes (not at all when P == 0 or F == 0, where nothing is launched), and one more kernel
 * behind the forward fills, for every pixel of the rendered tile rows,
 *   face  int32 [B,K,H,W]    the faces the pixel BLENDED, in blend order (front to back), -1 in unused slots;
 *   bary  fp32  [B,K,2,H,W]  the clamped barycentrics (u_c, v_c) the forward interpolated that face's vertex attributes
 *                            with -- weights (1 - u_c - v_c, u_c, v_c) for the face's three vertices --, 0 in unused slots;
 *   count int32 [B,H,W]      the number of blended faces of the pixel; it may exceed K: the pairs beyond K are counted,
 *                            not stored;
 * back to back in that order.  A blended pair is a covered (pixel, face) pair below the pixel's last contributor that the
 * forward did not skip (a degenerate ray-plane intersection is skipped, cuda_rasterizer/forward.cu:429-430): with opacities
 * o_k the pixel's blend weights are w_k = o_k prod_{j<k} (1 - o_j), its colour sum_k w_k c_k + T bg with T = prod_k (1 - o_k),
 * when count <= K.  Pixels outside the rendered tile rows are untouched, and nothing is written when P == 0 or F == 0: the
 * caller initialises the buffer (face -1, the rest 0) where that can happen, as it does for the images.  The values describe
 * the colour the call returns (after a redo, the redo's).  The images, the four scratch buffers and the backward are exactly
 * those of a call without the flag; no host wait is added (DMR_FLAG_ASYNC and stream capture work as before).  The tet
 * renderer's: DMR_FLAG_TET_FRAGMENTS. */
#define DMR_FLAG_TRI_FRAGMENTS 64
/* dmr_tri_backward only (ignored by every other call): the gradient of the fragment lists' barycentrics reaches the vertex
 * positions and, with DMR_FLAG_TRI_CAMERA_GRADS, the inverse matrices.  K travels in bits 8-15 of the flags as for the forward
 * (DMR_FRAGMENTS_K; the flag with K = 0 or K > 32 is an error, raised before anything is allocated or launched).  The call then
 * requests two more buffers through `alloc`, once each -- INPUTS, which the caller has filled before the call:
 *   DMR_BUF_TRI_FRAGMENT_FACES       int32 [B,K,H,W]    4 BKWH bytes, exactly: the face of every (pixel, slot) pair, as the forward
 *                                                       returned it -- or any other face: the pair need not be one the forward blended;
 *   DMR_BUF_TRI_FRAGMENT_BARY_GRADS  fp32  [B,K,2,H,W]  8 BKWH bytes, exactly: dL/d(u_c, v_c) of that pair
 * (not at all when there is nothing to back-propagate: P == 0, F == 0, num_rendered <= 0 or an empty tile-row band; the term is
 * then zero).  One more kernel behind the hit-parallel one recomputes, for every pixel of the rendered tile rows and every one of
 * its K slots, the pair's Moeller-Trumbore (u, v) and clamp region from the pixel's ray with the forward's arithmetic, and adds
 * the exact derivative of (u_c, v_c) times the upstream gradient -- coverage, list order and the clamp region held fixed, as for
 * every gradient here -- into dL_dverts, whichever of the reference's, the exact or the camera gradients the other flags select,
 * and with DMR_FLAG_TRI_CAMERA_GRADS also, through the pixel's ray, into the DMR_BUF_TRI_CAMERA_GRADS result.  A slot whose face
 * lies outside [0, F) contributes nothing (-1, the forward's unused slots, and anything else), nor does a pair whose upstream
 * gradient is (0, 0), a pair the forward would skip (denom == 0) or a pixel outside the rendered tile rows.  Pairs beyond K were
 * never stored and get nothing.  The other four gradient outputs, the scratch buffers and the work space's size are those of a
 * call without the flag; no host wait is added (DMR_FLAG_ASYNC and stream capture work as before). */
#define DMR_FLAG_TRI_FRAGMENT_GRADS 128
#define DMR_FRAGMENTS_K(flags) (((flags) >> 8) & 255)
#define DMR_FRAGMENTS_FLAGS(k) (DMR_FLAG_TRI_FRAGMENTS | (((k) & 255) << 8))
/* dmr_tet_forward only (ignored by every other call, as the tet calls ignore DMR_FLAG_TRI_FRAGMENTS): the tet renderer's
 * per-pixel fragment lists, in exact march order.  The bit lies outside bits 8-15, which carry K exactly as for the tri flag:
 * flags |= DMR_TET_FRAGMENTS_FLAGS(K), K in 1..32, read back with DMR_FRAGMENTS_K (the flag with K = 0 or K > 32 is an error,
 * raised before anything is allocated or launched).  The call then requests buffer DMR_BUF_TET_FRAGMENTS through `alloc`,
 * once, of exactly 4 BWH (3K + 1) bytes (not at all when P == 0 or F == 0, where nothing marches), and one more kernel behind
 * the march fills, for every pixel of the rendered tile rows,
 *   face  int32 [B,K,H,W]    the faces the pixel's march composited, in march order (front to back), -1 in unused slots;
 *   bary  fp32  [B,K,2,H,W]  the (u, v) of the pixel's ray on that face (Moeller-Trumbore, as the march evaluates it) --
 *                            weights (1 - u - v, u, v) for the face's three vertices --, UNCLAMPED: a face the march crosses
 *                            is hit in its interior by construction; 0 in unused slots;
 *   count int32 [B,H,W]      the pixel's number of march steps (n_contrib) where the march reached a valid end (out_active
 *                            == 1), 0 elsewhere; it may exceed K: the faces beyond K are counted, not stored;
 * back to back in that order.  A pixel whose march fails after some steps returns the bare background and has NO fragments.
 * Every counted face k was blended with weight T_k o_k, T_k the transmittance in front of it: T_0 = 1, T_{k+1} = T_k (1 - o_k)
 * -- with ONE exception: behind a face of opacity 1 the renderer goes on with T = T_EPS / 10 = 1e-5, not 0 (the march ends
 * there, since T < T_EPS: such a face is the pixel's last, and T_EPS / 10 is what multiplies the background).  The pixel's
 * colour is sum_k T_k o_k c_k + T bg when count <= K.  Pixels outside the rendered tile rows are untouched, and nothing is
 * written when P == 0 or F == 0: the caller initialises the buffer (face -1, the rest 0) where that can happen, as it does
 * for the images.  The values describe the images the call returns (after a redo, the redo's).  The kernel reads the first K
 * entries of the march sequence the forward leaves for the backward, so the call sizes that sequence to at least K rounded up
 * to a multiple of 4 steps (see the footprints: the binning buffer may be larger than without the flag, in the first call of a
 * view configuration above all; a K whose sequence alone exceeds 16 GiB fails before anything is launched).  The images, the
 * other three scratch buffers, the backward -- which decides on the device whether the sequence is complete, as before -- and
 * the estimate left for the next call are exactly those of a call without the flag; no host wait is added (DMR_FLAG_ASYNC and
 * stream capture work as before).  The barycentrics' gradient is the backward's DMR_FLAG_TET_FRAGMENT_GRADS. */
#define DMR_FLAG_TET_FRAGMENTS (1 << 16)
#define DMR_TET_FRAGMENTS_FLAGS(k) (DMR_FLAG_TET_FRAGMENTS | (((k) & 255) << 8))
/* dmr_tet_backward only (ignored by every other call): the gradient of the tet fragment lists' barycentrics reaches the vertex
 * positions and, with DMR_FLAG_TET_CAMERA_GRADS, the inverse matrices.  Implies DMR_FLAG_TET_FULL_GRADS (dL_dverts exists at
 * that level only: the call requests DMR_BUF_TET_GRADS and the images' own gradient fills it as with that flag).  K travels in
 * bits 8-15 of the flags (DMR_FRAGMENTS_K; the flag with K = 0 or K > 32 is an error, raised before anything is requested or
 * launched, whatever the scene; without the flag the K bits are ignored).  The call then requests two more buffers through
 * `alloc`, once each -- INPUTS, which the caller has filled before the call:
 *   DMR_BUF_TET_FRAGMENT_FACES       int32 [B,K,H,W]    4 BKWH bytes, exactly: the face of every (pixel, slot) pair, as the forward
 *                                                       returned it -- or any other face: the pair need not be one the march crossed;
 *   DMR_BUF_TET_FRAGMENT_BARY_GRADS  fp32  [B,K,2,H,W]  8 BKWH bytes, exactly: dL/d(u, v) of that pair
 * (not at all when there is nothing to back-propagate: P == 0, F == 0 or an empty tile-row band; the term is then zero).  One
 * more kernel behind the march's backward recomputes, for every pixel of the rendered tile rows and every one of its K slots,
 * the pair's unclamped Moeller-Trumbore (u, v) on the pixel's ray -- the forward's ray: origin inv_mv's translation column,
 * direction w / max(|w|, 1e-4), the seeded jitter a constant -- and adds the exact derivative of (u, v) times the upstream
 * gradient into the dL_dverts part of DMR_BUF_TET_GRADS and, with DMR_FLAG_TET_CAMERA_GRADS, through the ray into the dL/dinv_mv |
 * dL/dinv_proj half of DMR_BUF_TET_CAMERA_GRADS ((u, v) read the inverse matrices only: the dL/dmv | dL/dproj half gains
 * nothing).  There is no clamp and so no clamp region.  A slot whose face lies outside [0, F) contributes nothing, nor does a
 * pair whose upstream gradient is (0, 0), a pair with denom == 0 or a pixel outside the rendered tile rows; whether the pixel's
 * march was valid (out_active) is not consulted.  Pairs beyond K were never stored and get nothing.  The other outputs, the
 * scratch buffers, the work space and the march-sequence estimate are those of a call with DMR_FLAG_TET_FULL_GRADS (and the
 * camera flag) alone; no host wait is added (DMR_FLAG_ASYNC and stream capture work as before). */
#define DMR_FLAG_TET_FRAGMENT_GRADS (1 << 17)
/* 1 if an asynchronous / captured call on `device` (-1: the current one) overflowed its capacity since the flag was
 * last reset; call it after the stream (or the graph launch) has completed.  reset != 0 clears the flag. */
int dmr_overflowed(int device, int reset);
/* How often a default call had to enqueue stages a second time because its size estimate was too small (process-wide,
 * monotonic): 0 in a steady training loop; a figure that keeps growing says the estimates do not fit the workload (they are
 * kept per view configuration and power-of-two bucket of B * F). */
uint64_t dmr_redo_count(void);

/* out_color [B,3,H,W], out_depth [B,1,H,W] ([B,2,H,W] with DMR_FLAG_ALPHA: depth | alpha): every pixel of the rendered tile rows is written; the caller
 * zero-initialises them (render.cu:88-89) when a band leaves rows untouched or when P == 0 / F == 0
 * (nothing is launched, render.cu:105).  *num_rendered receives R = sum of tiles touched.
 * With DMR_FLAG_TRI_FRAGMENTS also the fragment lists, in a buffer requested through `alloc` (see the flag). */
int dmr_tri_forward(const dmr_scene* scene, float* out_color, float* out_depth,
                    dmr_alloc_fn alloc, void* alloc_ctx, void* stream, int* num_rendered);

/* Gradient outputs are fully overwritten: dL_dverts [P,3], dL_dvcolor [P,3],
 * dL_dfopacity [F], dL_dvdepth [B,P], dL_dfintense [B,F].
 * With DMR_FLAG_TRI_EXACT_GRADS in scene->flags, dL_dverts is the exact derivative of colour and depth through each blended
 * pair's Moeller-Trumbore (u, v) (coverage, list order and the clamp region held fixed, as for every gradient here); the
 * other four outputs are the same sums in another order.  With DMR_FLAG_TRI_CAMERA_GRADS the call also requests buffer
 * DMR_BUF_TRI_CAMERA_GRADS through `alloc`, once, of 128 B bytes, and fully overwrites it with fp32
 * [B][dL/dinv_mv 16 | dL/dinv_proj 16] in the contract layout m[4*col+row] whatever mats_transposed says: the gradients of
 * the inverse matrices through every pixel's ray (origin = inv_mv's translation column, direction
 * normalize(inv_mv (inv_proj (ndc, -1, 1)).xyz - origin) with no w divide); their w rows are 0.  dL_dvdepth does not
 * involve the matrices.  No host wait is added (DMR_FLAG_ASYNC and stream capture work as without the flags).  Without
 * the flags the call is exactly as before and requests no buffer beyond the work space.
 * With DMR_FLAG_ALPHA dL_ddepth is [B,2,H,W] (dL/ddepth | dL/dalpha); only dL_dfopacity gains a term.
 * With DMR_FLAG_TRI_FRAGMENT_GRADS dL_dverts (and the camera gradients) gain the fragment lists' term, from two input buffers
 * requested through `alloc` (see the flag). */
int dmr_tri_backward(const dmr_scene* scene, const float* dL_dcolor, const float* dL_ddepth,
                     int num_rendered, const void* point_buf, const void* face_buf,
                     const void* binning_buf, const void* image_buf,
                     float* dL_dverts, float* dL_dvcolor, float* dL_dfopacity,
                     float* dL_dvdepth, float* dL_dfintense,
                     dmr_alloc_fn alloc, void* alloc_ctx, void* stream);

/* out_active [B,H,W]: 1.0 where the ray marched to a valid end, else 0.0.  Like the tri forward, every pixel of the
 * rendered tile rows of all three outputs is written (background / 1 / 0 where the march fails).  With DMR_FLAG_ALPHA
 * out_depth is [B,2,H,W] (depth | alpha; alpha 0 where the march fails).
 * With DMR_FLAG_TET_FRAGMENTS also the fragment lists, in a buffer requested through `alloc` (see the flag). */
int dmr_tet_forward(const dmr_scene* scene, float* out_color, float* out_depth, float* out_active,
                    dmr_alloc_fn alloc, void* alloc_ctx, void* stream, int* num_rendered);

/* dL_dvcolor [P,3], dL_dfopacity [F], fully overwritten.
 * With DMR_FLAG_TET_FULL_GRADS in scene->flags, the call also requests buffer DMR_BUF_TET_GRADS through `alloc`, once, of
 * 4 (3P + BF) bytes, and fully overwrites it with [dL_dverts [P,3] | dL_dfintense [B,F]] (fp32): the gradients of the
 * vertex positions and face intensities along the forward's march (each marched face enters through its hit (t, u, v):
 * u, v set the interpolated colour, t the hit point's ndc depth; opacities and transmittance do not depend on the
 * positions).  The buffer is caller-owned like the others; no host wait is added (DMR_FLAG_ASYNC and stream capture work
 * as without the flag).  verts_depth gets no gradient (the tet renderer does not read it).
 * With DMR_FLAG_TET_CAMERA_GRADS (implies DMR_FLAG_TET_FULL_GRADS) the call also requests buffer DMR_BUF_TET_CAMERA_GRADS
 * through `alloc`, once, of 256 B bytes, and fully overwrites it with fp32 [B][dL/dinv_mv 16 | dL/dinv_proj 16 | dL/dmv 16 |
 * dL/dproj 16] in the contract layout m[4*col+row] whatever mats_transposed says.  The inverse matrices enter through every
 * pixel's ray (origin = inv_mv's translation column, direction normalize(inv_mv (inv_proj (ndc, -1, 1)).xyz - origin) with
 * no w divide and the length clamped to 1e-4, the seeded jitter held fixed); mv and proj through the ndc depth of each
 * marched face's hit point (rows 0-2 of mv, rows 2-3 of proj).  The w rows of the inverses get 0.  Per-tile partials go to
 * a DMR_BUF_WORK request.  No host wait is added.  Without the flags the call is exactly as before and requests no buffer.
 * With DMR_FLAG_ALPHA dL_ddepth is [B,2,H,W] (dL/ddepth | dL/dalpha); only dL_dfopacity gains a term.
 * With DMR_FLAG_TET_FRAGMENT_GRADS (implies DMR_FLAG_TET_FULL_GRADS) dL_dverts (and the inverse matrices' camera gradients) gain
 * the fragment lists' term, from two input buffers requested through `alloc` (see the flag). */
int dmr_tet_backward(const dmr_scene* scene, const float* dL_dcolor, const float* dL_ddepth,
                     const void* point_buf, const void* face_buf,
                     const void* binning_buf, const void* image_buf,
                     float* dL_dvcolor, float* dL_dfopacity,
                     dmr_alloc_fn alloc, void* alloc_ctx, void* stream);

/* Caller-side step of the path: the reference wrapper computes th.inverse of the (transposed) model-view and
 * projection matrices on every forward (dmesh_renderer/__init__.py:62-63,298-299) -- on a GPU that is two batched
 * LU factorisations, ~0.12 ms of small kernels.  This inverts `count` 4x4 matrices with one kernel (adjugate /
 * determinant in double precision, rounded to fp32 once): out[16*m + 4*i + j] = inverse(A_m)[i][j] with
 * A_m[i][j] = in[16*m + 4*i + j], or in[16*m + i + 4*j] when `transposed` (the storage behind a .transpose(1, 2)
 * view).  A singular matrix gives inf/nan entries, as a division by a zero determinant does. */
int dmr_invert_mats(const float* in, int count, int transposed, float* out, void* stream);

/* Parity/debug export of forward intermediates held in the scratch buffers.
 * name: "image" (f32 [B*P,2]) "ndc_z" (f32 [B*P]) "key_depth" (f32 [B*F]) "max_depth" (tet, f32 [B*F])
 * "tiles_touched" (u32 [B*F]) "ranges" (u32 [B*Nt,2]) "face_list" (u32 [R]) "final_T" "final_prev_T"
 * (f32 [B*W*H]) "n_contrib" (u32 [B*W*H]) "tile_hits" (tri, u32 [B*Nt]: blended (pixel, face) pairs per tile) "first_face" "first_tet" "last_face" "last_tet" (i32, tet)
 * "is_active" (u8, tet) "tet_seq" (tet, u32 [2]: the longest march in steps, the steps per pixel the forward's march sequence had room for).  dst is a DEVICE pointer with room for `cap` bytes.  Returns the byte size
 * of the item (copying min(size, cap) when dst != NULL), or -1. */
int64_t dmr_export(const dmr_scene* scene, int is_tet, int num_rendered, const char* name,
                   const void* point_buf, const void* face_buf, const void* binning_buf,
                   const void* image_buf, void* dst, int64_t cap, void* stream);

/* Per-stage device timing with HIP events recorded on the caller's stream (bench.py's roofline
 * leg).  `mask` has bit i set to time stage i; 0 disables (the default: no events recorded). */
enum {
    DMR_STAGE_PROJECT = 0, DMR_STAGE_SETUP_FACES = 1, DMR_STAGE_SCAN = 2, DMR_STAGE_SCATTER = 3,
    DMR_STAGE_SORT = 4, DMR_STAGE_TRI_FORWARD = 5, DMR_STAGE_TRI_BACKWARD = 6, DMR_STAGE_TRI_UNPACK = 7,
    DMR_STAGE_TET_FIRST = 8, DMR_STAGE_TET_FORWARD = 9, DMR_STAGE_TET_BACKWARD = 10,
    DMR_STAGE_TRI_BACKWARD_HITS = 11, DMR_NUM_STAGES = 12
};
void dmr_profile_enable(uint32_t mask);
/* Waits for the recorded events, ADDS each stage's elapsed milliseconds / launch count into
 * ms[DMR_NUM_STAGES] / launches[DMR_NUM_STAGES] and clears the records.  Returns 0 on success. */
int dmr_profile_collect(double* ms, int64_t* launches);
const char* dmr_stage_name(int stage);

const char* dmr_last_error(void);
int dmr_abi_version(void);
/* Name of the code object architecture the library was built for ("gfx950"). */
const char* dmr_build_arch(void);

#ifdef __cplusplus
}
#endif
#endif /* DMESH_RENDERER_AMD_H */
