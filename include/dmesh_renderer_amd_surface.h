/* dmesh_renderer_amd_surface.h -- the surface frame of packed rows: hit point, geometric normal turned towards the camera,
 * mirrored view ray.
 *
 * A companion of dmesh_renderer_amd.h (same library, libdmesh_renderer_hip.so; errors are read through its
 * dmr_last_error()) and of dmesh_renderer_amd_packed.h, whose lists, `row`, `n_used` and slot rules it takes as they are: a slot
 * COUNTS when 0 <= row[slot] < N and its face id lies in [0, F), so a `row` made for another F or capacity never reads or
 * writes out of bounds.  The view of a slot is its b: no row-to-view map is needed.  For a counting slot (b, k, y, x) with
 * (i0, i1, i2) = faces[f], p_j = verts[i_j] and (u, v) = bary[b, k, :, y, x], in float32:
 *
 *   h = (1 - u - v) p0 + u p1 + v p2            dmr_interpolate_packed's expression: hit is its out for vert_attrs = verts, bit for bit
 *   e1 = p1 - p0, e2 = p2 - p0, g = e1 x e2, a = |g|, m = g / a
 *                                               m = 0 when a is not finite or a < 1e-20 (a degenerate face): nothing then
 *                                               flows into verts through the normal
 *   w = h - origin[b], len = |w|, d = w / len   d = 0 when len is not finite or len < 1e-8 (dmr_sh_rows' rule and constant)
 *   s = m . d
 *   normal  = m if s <= 0, else -m              the unit geometric normal turned towards the camera: normal . d <= 0 whatever
 *                                               the winding of the face.  The sign is a constant of every gradient.
 *   reflect = d - 2 s m                         the mirrored view ray: unit length, independent of the winding; d on a
 *                                               degenerate face, 0 where d = 0
 *
 * hit, normal and reflect are rows [N,3] at row[slot].  A counting slot whose face names a vertex outside [0, P) gives three
 * rows of exact zeros and no gradient.  Rows min(n_used[0], N) .. N - 1 are exact zeros in all three; rows below n_used[0]
 * that no slot holds are left unwritten (`row` is expected to come from dmr_pack_slots on the same lists).
 *
 * Backward, with Gh, Gn, Gr the upstream rows of a counting slot and sigma = +-1 the sign chosen above:
 *   dL/dm = sigma Gn - 2 s Gr - 2 (m . Gr) d           dL/dd = Gr - 2 (m . Gr) m
 *   dL/dg = (dL/dm - m (m . dL/dm)) / a  (0 on a degenerate face)
 *   dL/dw = (dL/dd - d (d . dL/dd)) / len  (0 where d = 0)
 *   dL/dh = Gh + dL/dw                                  dL/dorigin[b] -= dL/dw
 *   dL/de1 = e2 x dL/dg                                 dL/de2 = dL/dg x e1
 *   dL/dp0 = (1 - u - v) dL/dh - dL/de1 - dL/de2        dL/dp1 = u dL/dh + dL/de1        dL/dp2 = v dL/dh + dL/de2
 *   dL/du = e1 . dL/dh                                  dL/dv = e2 . dL/dh
 *
 * Both rules test the float32 values: a = sqrt(g . g) and len = sqrt(w . w) as float32 compute them, so a face whose g . g
 * underflows to 0 (|g| below about 1e-19) or overflows (above about 1e19) is degenerate here though float64 would not call it
 * so; vertices in a unit box are far from both.  The backward recomputes the frame: sigma is the sign of ITS s, which is the
 * forward's except, possibly, where |s| lies within rounding of 0 (about 1e-7) -- there `normal` itself is decided by rounding.
 *
 * 1 <= K <= 32, 0 <= N.  Offsets into the [N,3] buffers are 64-bit.  Both calls only enqueue on `stream`: no host wait, no
 * allocation, safe to capture into a HIP graph.  Every output is fully overwritten (what is accumulated into is zeroed on the
 * stream first, by a kernel).  All pointers are device pointers.
 * Return value: 0 on success, non-zero on error; dmr_last_error() then returns a description.  The first check that fails
 * decides it, in this order: the sizes (B, H, W, P, F; K), "bad rows" (N below 0), null lists (face, bary, row), null faces
 * (when F > 0), null verts / origin (verts when F > 0 and P > 0), null n_used, "problem too large" (B K H W, B F or a launch
 * grid at 2^31 or above) -- and only then what a single call asks for: a null output (the forward, when N > 0); all three
 * upstreams null (the backward, when N > 0); no gradient wanted (the backward: returns 0 and enqueues nothing).  Every check
 * precedes every launch.
 */
#ifndef DMESH_RENDERER_AMD_SURFACE_H
#define DMESH_RENDERER_AMD_SURFACE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* face i32 [B,K,H,W], bary f32 [B,K,2,H,W], row i32 [B,K,H,W], n_used i32 [1], faces i32 [F,3], verts f32 [P,3], origin f32 [B,3]
 * -> hit, normal, reflect f32 [N,3].  One launch.  N == 0: returns 0 and enqueues nothing. */
int dmr_surface_packed(int B, int K, int H, int W, int P, int F, int N, const int32_t* face, const float* bary, const int32_t* row,
                       const int32_t* n_used, const int32_t* faces, const float* verts, const float* origin, float* hit,
                       float* normal, float* reflect, void* stream);

/* The gradients of the three outputs.  grad_hit, grad_normal, grad_reflect f32 [N,3] are the upstream gradients; any may be
 * null (zero, and costs nothing), but not all three when N > 0.  They are not read in rows no counting slot holds.  Each of the
 * three outputs may be null (not wanted, and then not computed): dL_dverts f32 [P,3]; dL_dbary f32 [B,K,2,H,W], an exact 0 in
 * slots that do not count; dL_dorigin f32 [B,3].  N == 0: the outputs that are wanted are written as zeros. */
int dmr_surface_packed_backward(int B, int K, int H, int W, int P, int F, int N, const int32_t* face, const float* bary,
                                const int32_t* row, const int32_t* n_used, const int32_t* faces, const float* verts,
                                const float* origin, const float* grad_hit, const float* grad_normal, const float* grad_reflect,
                                float* dL_dverts, float* dL_dbary, float* dL_dorigin, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DMESH_RENDERER_AMD_SURFACE_H */
