/* dmesh_renderer_amd_shade.h -- shading over per-pixel fragment lists: the fused compositing of per-vertex attributes.
 *
 * A companion of dmesh_renderer_amd.h (same library, libdmesh_renderer_hip.so; errors are read through its
 * dmr_last_error()).  The two calls here take no dmr_scene and none of the scratch buffers: they read the fragment lists a
 * renderer wrote (DMR_FLAG_TRI_FRAGMENTS / DMR_FLAG_TET_FRAGMENTS), or lists the caller made, and plain tensors.
 *
 * Per pixel (b, y, x), over the K slots k = 0..K-1 of its list, front to back:
 *     o_k = faces_opacity[face_k]            T_0 = 1, T_{k+1} = T_k (1 - o_k)          w_k = T_k o_k
 *     a_k = (1 - u - v) A[v0] + u A[v1] + v A[v2]      (v0, v1, v2) = faces[face_k], (u, v) = bary[b, k, :, y, x], A = vert_attrs
 *     s_k = face_scale[b, face_k]  (1 when face_scale is null)
 *     image = sum_k w_k s_k a_k  [B,C,H,W]              T = T_K  [B,1,H,W]
 * A slot whose face id lies outside [0, F) is empty (o = 0, contributes nothing) wherever it sits in the list; the lists'
 * count is not read.  1 <= K <= 32, 1 <= C <= 256.
 *
 * Both calls only enqueue on `stream`: no host wait, no allocation, safe to capture into a HIP graph.  Every output is
 * fully overwritten (what is accumulated into is zeroed on the stream first).  All pointers are device pointers.
 * Return value: 0 on success, non-zero on error; dmr_last_error() then returns a description.
 */
#ifndef DMESH_RENDERER_AMD_SHADE_H
#define DMESH_RENDERER_AMD_SHADE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* face i32 [B,K,H,W], bary f32 [B,K,2,H,W], faces i32 [F,3], faces_opacity f32 [F], vert_attrs f32 [P,C],
 * face_scale f32 [B,F] or null -> image f32 [B,C,H,W], T f32 [B,H,W]. */
int dmr_composite_fragments(int B, int K, int H, int W, int P, int F, int C, const int32_t* face, const float* bary,
                            const int32_t* faces, const float* faces_opacity, const float* vert_attrs, const float* face_scale,
                            float* image, float* T, void* stream);

/* The gradients of the above.  grad_image f32 [B,C,H,W] and grad_T f32 [B,H,W] are the upstream gradients; either may be
 * null (zero).  Each of the four outputs may be null (not wanted, and then not computed):
 *     dL_dfaces_opacity f32 [F], dL_dvert_attrs f32 [P,C], dL_dface_scale f32 [B,F] (needs face_scale),
 *     dL_dbary f32 [B,K,2,H,W] (0 in empty slots). */
int dmr_composite_fragments_backward(int B, int K, int H, int W, int P, int F, int C, const int32_t* face, const float* bary,
                                     const int32_t* faces, const float* faces_opacity, const float* vert_attrs,
                                     const float* face_scale, const float* grad_image, const float* grad_T,
                                     float* dL_dfaces_opacity, float* dL_dvert_attrs, float* dL_dface_scale, float* dL_dbary,
                                     void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DMESH_RENDERER_AMD_SHADE_H */
