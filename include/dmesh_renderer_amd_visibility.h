/* dmesh_renderer_amd_visibility.h -- shading over per-pixel fragment lists: per-face visibility and coverage.
 *
 * A companion of dmesh_renderer_amd.h (same library, libdmesh_renderer_hip.so; errors are read through its
 * dmr_last_error()).  The two calls here take no dmr_scene and none of the scratch buffers: they read the face ids of the
 * fragment lists a renderer wrote (DMR_FLAG_TRI_FRAGMENTS / DMR_FLAG_TET_FRAGMENTS), or of lists the caller made, and the
 * opacities.  No barycentrics, no faces, no vertices.
 *
 * Per pixel (b, y, x), over the K slots k = 0..K-1 of its list, front to back, with f_k = face[b, k, y, x]:
 *     o_k = faces_opacity[f_k]            T_0 = 1, T_{k+1} = T_k (1 - o_k)          w_k = T_k o_k
 *     p   = pixel_weight[b, y, x]         (1 when pixel_weight is null)
 *     vis[b, f]        = sum over the (pixel, slot) pairs with f_k == f of p w_k
 *     max_weight[b, f] = max(0, max over the same pairs of w_k)                      (without p)
 *     pixels[b, f]     = the number of those pairs, whatever their weight
 * A slot whose face id lies outside [0, F) is empty (o = 0, contributes nothing) wherever it sits in the list; the lists'
 * count is not read.  1 <= K <= 32, K * H * W < 2^31.
 *
 * Both calls only enqueue on `stream`: no host wait, no allocation, safe to capture into a HIP graph.  Every output is
 * fully overwritten (what is accumulated into is zeroed on the stream first).  All pointers are device pointers.
 * Return value: 0 on success, non-zero on error; dmr_last_error() then returns a description.
 */
#ifndef DMESH_RENDERER_AMD_VISIBILITY_H
#define DMESH_RENDERER_AMD_VISIBILITY_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* face i32 [B,K,H,W], faces_opacity f32 [F], pixel_weight f32 [B,H,W] or null -> vis f32 [B,F]; max_weight f32 [B,F] and
 * pixels i32 [B,F]: both or neither (null: not wanted, and then not computed). */
int dmr_face_visibility(int B, int K, int H, int W, int F, const int32_t* face, const float* faces_opacity,
                        const float* pixel_weight, float* vis, float* max_weight, int32_t* pixels, void* stream);

/* The gradients of vis.  grad_vis f32 [B,F] is the upstream gradient.  Each of the two outputs may be null (not wanted, and
 * then not computed): dL_dfaces_opacity f32 [F], dL_dpixel_weight f32 [B,H,W] (needs pixel_weight).  With G_k = grad_vis[b, f_k]
 * (0 in empty slots): R_{K-1} = 0, R_{k-1} = o_k G_k + (1 - o_k) R_k, dL/do_k = p T_k (G_k - R_k), dL/dp = sum_k w_k G_k;
 * nothing divides by 1 - o. */
int dmr_face_visibility_backward(int B, int K, int H, int W, int F, const int32_t* face, const float* faces_opacity,
                                 const float* pixel_weight, const float* grad_vis, float* dL_dfaces_opacity,
                                 float* dL_dpixel_weight, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DMESH_RENDERER_AMD_VISIBILITY_H */
