/* dmesh_renderer_amd_deferred.h -- shading over per-pixel fragment lists: the two ends of a deferred shader.
 *
 * A companion of dmesh_renderer_amd.h (same library, libdmesh_renderer_hip.so; errors are read through its
 * dmr_last_error()).  The four calls here take no dmr_scene and none of the scratch buffers: they read the fragment lists a
 * renderer wrote (DMR_FLAG_TRI_FRAGMENTS / DMR_FLAG_TET_FRAGMENTS), or lists the caller made.  Between the two pairs the
 * caller runs code of its own on every fragment:
 *
 *   interpolate   per-vertex attributes at every fragment, out[b, k, c, y, x], with f_k = face[b, k, y, x], (u, v) = bary[b, k, :, y, x]
 *                 and (v0, v1, v2) = faces[f_k]:
 *                     out = (1 - u - v) A[v0] + u A[v1] + v A[v2]
 *                 0 in an empty slot, and 0 where one of the three is no row of vert_attrs.
 *   composite     the front-to-back blend of per-slot values the caller computed, values[b, k, c, y, x]:
 *                     o_k = faces_opacity[f_k]      T_0 = 1, T_{k+1} = T_k (1 - o_k)      w_k = T_k o_k
 *                     s_k = face_scale[b, f_k]      (1 when face_scale is null)
 *                     image[b, c, y, x] = sum_k w_k s_k values[b, k, c, y, x]             T[b, 0, y, x] = T_K
 *                 The value of an empty slot is not read.  A slot of weight 0 that is not empty (opacity 0, or behind a face
 *                 of opacity 1) may or may not be read: what a non-finite value there gives is unspecified.
 *
 * A slot whose face id lies outside [0, F) is empty wherever it sits in the list; the lists' count is not read.
 * 1 <= K <= 32, 1 <= C <= 256.  Offsets into values, out and their gradients are 64-bit: B K C H W may pass 2^31.
 *
 * All four calls only enqueue on `stream`: no host wait, no allocation, safe to capture into a HIP graph.  Every output is
 * fully overwritten (what is accumulated into is zeroed on the stream first, by a kernel).  All pointers are device pointers.
 * Return value: 0 on success, non-zero on error; dmr_last_error() then returns a description.  The first check that fails
 * decides it, in this order: the sizes (B, H, W, P, F; K; C), null lists, null faces / faces_opacity, null vert_attrs / values,
 * "problem too large" (K H W, B F or a launch grid at 2^31 or above) -- and only then what a single call asks for: a null output,
 * a null grad_out, dL_dface_scale without face_scale (as in the other shading headers' calls, where the size limits also come
 * before the null-output check).
 */
#ifndef DMESH_RENDERER_AMD_DEFERRED_H
#define DMESH_RENDERER_AMD_DEFERRED_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* face i32 [B,K,H,W], bary f32 [B,K,2,H,W], faces i32 [F,3], vert_attrs f32 [P,C] -> out f32 [B,K,C,H,W]. */
int dmr_interpolate_fragments(int B, int K, int H, int W, int P, int F, int C, const int32_t* face, const float* bary,
                              const int32_t* faces, const float* vert_attrs, float* out, void* stream);

/* The gradients of out.  grad_out f32 [B,K,C,H,W] is the upstream gradient.  Each of the two outputs may be null (not wanted,
 * and then not computed): dL_dvert_attrs f32 [P,C]; dL_dbary f32 [B,K,2,H,W] = ((A[v1] - A[v0]) . g_k, (A[v2] - A[v0]) . g_k),
 * an exact 0 in empty slots.  With neither the call returns 0 and enqueues nothing. */
int dmr_interpolate_fragments_backward(int B, int K, int H, int W, int P, int F, int C, const int32_t* face, const float* bary,
                                       const int32_t* faces, const float* vert_attrs, const float* grad_out,
                                       float* dL_dvert_attrs, float* dL_dbary, void* stream);

/* face i32 [B,K,H,W], faces_opacity f32 [F], values f32 [B,K,C,H,W], face_scale f32 [B,F] or null
 * -> image f32 [B,C,H,W], T f32 [B,1,H,W]. */
int dmr_composite_values(int B, int K, int H, int W, int F, int C, const int32_t* face, const float* faces_opacity,
                         const float* values, const float* face_scale, float* image, float* T, void* stream);

/* The gradients of image and T.  grad_image f32 [B,C,H,W] and grad_T f32 [B,1,H,W] are the upstream gradients; either may be
 * null (zero; without grad_image no value is read).  Each of the three outputs may be null (not wanted, and then not
 * computed): dL_dfaces_opacity f32 [F], dL_dvalues f32 [B,K,C,H,W] (0 in empty slots), dL_dface_scale f32 [B,F] (needs
 * face_scale).  With g, gT the pixel's upstreams, e_k = values_k . g and d_k = s_k e_k: dL/dvalues_k = w_k s_k g;
 * R_{K-1} = gT, R_{k-1} = o_k d_k + (1 - o_k) R_k, dL/do_k = T_k (d_k - R_k), dL/ds_k = w_k e_k; nothing divides by 1 - o.
 * With no output wanted the call returns 0 and enqueues nothing. */
int dmr_composite_values_backward(int B, int K, int H, int W, int F, int C, const int32_t* face, const float* faces_opacity,
                                  const float* values, const float* face_scale, const float* grad_image, const float* grad_T,
                                  float* dL_dfaces_opacity, float* dL_dvalues, float* dL_dface_scale, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DMESH_RENDERER_AMD_DEFERRED_H */
