/* dmesh_renderer_amd_texture.h -- shading over per-pixel fragment lists: fused bilinear texture sampling and compositing.
 *
 * A companion of dmesh_renderer_amd.h and dmesh_renderer_amd_shade.h (same library, libdmesh_renderer_hip.so; errors are read
 * through dmr_last_error()).  The two calls here take no dmr_scene and none of the scratch buffers: they read the fragment
 * lists a renderer wrote (DMR_FLAG_TRI_FRAGMENTS / DMR_FLAG_TET_FRAGMENTS), or lists the caller made, and plain tensors.
 *
 * Per pixel (b, y, x), over the K slots k = 0..K-1 of its list, front to back (o_k, T_k, w_k, s_k as in
 * dmesh_renderer_amd_shade.h):
 *     (s, t)_k = (1 - u - v) UV[c0] + u UV[c1] + v UV[c2]      (c0, c1, c2) = uv_faces[face_k], (u, v) = bary[b, k, :, y, x]
 *     x = s Wt - 0.5, y = t Ht - 0.5, x0 = floor(x), fx = x - x0, likewise y          (texel centres at half-integers; t = 0 is
 *                                                                                      row 0 of the texture, no flip)
 *     ix0 = wrap(x0, Wt), ix1 = wrap(x0 + 1, Wt), likewise iy      wrap 0: clamp to [0, n-1];  wrap 1: remainder mod n (>= 0)
 *     c_k = (1-fy) ((1-fx) tex[iy0,ix0] + fx tex[iy0,ix1]) + fy ((1-fx) tex[iy1,ix0] + fx tex[iy1,ix1])
 *     image = sum_k w_k s_k c_k  [B,C,H,W]              T = T_K  [B,1,H,W]
 * fx, fy come from the unwrapped coordinate, the indices wrap afterwards.  Bilinear only: no mip levels, no nearest filter,
 * one texture for every view.  The texture is channel-last, f32 [Ht,Wt,C].
 *
 * A slot whose face id lies outside [0, F) is empty (o = 0, contributes nothing) wherever it sits in the list; the lists'
 * count is not read.  A face one of whose uv_faces entries is no row of vert_uvs samples nothing (its slot adds no colour and
 * receives no gradient but that of its opacity).  Texel indices are clamped into the texture as the last step before every
 * access: non-finite or huge UVs read and write in bounds; the value they produce is unspecified.
 * 1 <= K <= 32, 1 <= C <= 32, Ht, Wt >= 1, Ht * Wt * ceil(C / 4) < 2^32 - 1.
 *
 * Both calls only enqueue on `stream`: no host wait, no allocation, safe to capture into a HIP graph.  Every output is
 * fully overwritten (what is accumulated into is zeroed on the stream first).  All pointers are device pointers.
 * Return value: 0 on success, non-zero on error; dmr_last_error() then returns a description.
 */
#ifndef DMESH_RENDERER_AMD_TEXTURE_H
#define DMESH_RENDERER_AMD_TEXTURE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* face i32 [B,K,H,W], bary f32 [B,K,2,H,W], uv_faces i32 [F,3] (rows of vert_uvs per corner), faces_opacity f32 [F],
 * vert_uvs f32 [Pu,2], texture f32 [Ht,Wt,C], face_scale f32 [B,F] or null, wrap 0 = clamp / 1 = repeat
 * -> image f32 [B,C,H,W], T f32 [B,H,W]. */
int dmr_composite_texture(int B, int K, int H, int W, int Pu, int F, int C, int Ht, int Wt, int wrap, const int32_t* face,
                          const float* bary, const int32_t* uv_faces, const float* faces_opacity, const float* vert_uvs,
                          const float* texture, const float* face_scale, float* image, float* T, void* stream);

/* The gradients of the above.  grad_image f32 [B,C,H,W] and grad_T f32 [B,H,W] are the upstream gradients; either may be
 * null (zero).  Each of the five outputs may be null (not wanted, and then not computed):
 *     dL_dfaces_opacity f32 [F], dL_dvert_uvs f32 [Pu,2], dL_dtexture f32 [Ht,Wt,C], dL_dface_scale f32 [B,F] (needs
 *     face_scale), dL_dbary f32 [B,K,2,H,W] (0 in empty slots).
 * The texel cell (the floor) is held constant: where a sample sits on a texel-centre line the UV and barycentric gradients
 * are those of the cell it was put in. */
int dmr_composite_texture_backward(int B, int K, int H, int W, int Pu, int F, int C, int Ht, int Wt, int wrap, const int32_t* face,
                                   const float* bary, const int32_t* uv_faces, const float* faces_opacity, const float* vert_uvs,
                                   const float* texture, const float* face_scale, const float* grad_image, const float* grad_T,
                                   float* dL_dfaces_opacity, float* dL_dvert_uvs, float* dL_dtexture, float* dL_dface_scale,
                                   float* dL_dbary, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DMESH_RENDERER_AMD_TEXTURE_H */
