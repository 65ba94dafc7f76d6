/* dmesh_renderer_amd_packed.h -- deferred shading over per-pixel fragment lists on PACKED, channel-last rows.
 *
 * A companion of dmesh_renderer_amd.h (same library, libdmesh_renderer_hip.so; errors are read through its
 * dmr_last_error()) and the packed form of dmesh_renderer_amd_deferred.h: the used slots of the lists become rows 0 .. n - 1,
 * interpolation writes values[row, c] (row-major [N, C], what a linear layer takes), the caller's own code runs on the rows,
 * and the blend reads [N, C] rows back.  No dmr_scene and none of the scratch buffers.
 *
 *   pack          a slot is USED when its face id lies in [0, F).  Used slots are numbered in the order of the flattened
 *                 [B,K,H,W] lists, (b, k, y, x): row[slot] = the number of used slots before it, -1 in an empty slot, and -1 in
 *                 a used slot whose number is >= capacity (it is DROPPED, and is empty to every call below).  n_used[0] is
 *                 the number of used slots whatever the capacity: n_used[0] > capacity tells the caller that slots were dropped.
 *   interpolate   out[row, c] = (1 - u - v) A[v0][c] + u A[v1][c] + v A[v2][c] for every slot with a row, (v0, v1, v2) =
 *                 faces[f_k], (u, v) = bary[b, k, :, y, x]; a row of exact zeros where one of the three is no row of vert_attrs.
 *                 Rows min(n_used[0], N) .. N - 1 are exact zeros.
 *   composite     o_k = faces_opacity[f_k]      T_0 = 1, T_{k+1} = T_k (1 - o_k)      w_k = T_k o_k
 *                 s_k = face_scale[b, f_k]      (1 when face_scale is null)
 *                 image[b, c, y, x] = sum_k w_k s_k values[row_k, c]                    T[b, 0, y, x] = T_K
 *                 over the slots that COUNT.  A slot of weight 0 that counts (opacity 0, or behind a face of opacity 1) may or
 *                 may not be read: what a non-finite value there gives is unspecified.
 *
 * In the interpolate and composite calls a slot COUNTS only if 0 <= row[slot] < N AND its face id lies in [0, F): a `row`
 * made for another F, or for another capacity, never reads or writes out of bounds.  A slot with 0 <= row[slot] < N whose face
 * id is outside [0, F) (a `row` made with a larger F) is empty: interpolate writes its row as zeros, the blend skips it and
 * stores zeros in its row of dL_dvalues.  `row` is expected to come from dmr_pack_slots on the same lists: rows below n_used[0]
 * that no slot holds are left unwritten.
 * 1 <= K <= 32, 1 <= C <= 256, 0 <= N, 0 <= capacity.  Offsets into the [N, C] buffers are 64-bit: N C may pass 2^31.
 *
 * All five calls only enqueue on `stream`: no host wait, no allocation, safe to capture into a HIP graph.  Every output is
 * fully overwritten (what is accumulated into is zeroed on the stream first, by a kernel).  All pointers are device pointers.
 * Return value: 0 on success, non-zero on error; dmr_last_error() then returns a description.  The first check that fails
 * decides it, in this order: the sizes (B, H, W, P, F; K; C), "bad rows" (N or capacity below 0), null lists (face, bary, row),
 * null faces / faces_opacity, null vert_attrs / values (values only when N > 0), null n_used (the interpolate calls),
 * "problem too large" (B K H W, B F or a launch grid at 2^31 or above) -- and only then what a single call asks for: a null
 * output, a null grad_out (when N > 0), a null n_used (the blend's backward), dL_dface_scale without face_scale.
 */
#ifndef DMESH_RENDERER_AMD_PACKED_H
#define DMESH_RENDERER_AMD_PACKED_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* face i32 [B,K,H,W] -> row i32 [B,K,H,W], n_used i32 [1].  Three launches; no workgroup waits for another inside a kernel.
 * (`row` doubles as the scratch of the scan: nothing else is needed.) */
int dmr_pack_slots(int B, int K, int H, int W, int F, int capacity, const int32_t* face, int32_t* row, int32_t* n_used, void* stream);

/* face i32 [B,K,H,W], bary f32 [B,K,2,H,W], row i32 [B,K,H,W], n_used i32 [1], faces i32 [F,3], vert_attrs f32 [P,C]
 * -> out f32 [N,C].  N == 0: returns 0 and enqueues nothing. */
int dmr_interpolate_packed(int B, int K, int H, int W, int P, int F, int C, int N, const int32_t* face, const float* bary,
                           const int32_t* row, const int32_t* n_used, const int32_t* faces, const float* vert_attrs, float* out,
                           void* stream);

/* The gradients of out.  grad_out f32 [N,C] is the upstream gradient (not read in rows no counting slot holds).  Each of the
 * two outputs may be null (not wanted, and then not computed): dL_dvert_attrs f32 [P,C]; dL_dbary f32 [B,K,2,H,W] =
 * ((A[v1] - A[v0]) . g_k, (A[v2] - A[v0]) . g_k), an exact 0 in empty and dropped slots.  With neither the call returns 0 and
 * enqueues nothing. */
int dmr_interpolate_packed_backward(int B, int K, int H, int W, int P, int F, int C, int N, const int32_t* face, const float* bary,
                                    const int32_t* row, const int32_t* n_used, const int32_t* faces, const float* vert_attrs,
                                    const float* grad_out, float* dL_dvert_attrs, float* dL_dbary, void* stream);

/* face i32 [B,K,H,W], row i32 [B,K,H,W], faces_opacity f32 [F], values f32 [N,C], face_scale f32 [B,F] or null
 * -> image f32 [B,C,H,W], T f32 [B,1,H,W]. */
int dmr_composite_values_packed(int B, int K, int H, int W, int F, int C, int N, const int32_t* face, const int32_t* row,
                                const float* faces_opacity, const float* values, const float* face_scale, float* image, float* T,
                                void* stream);

/* The gradients of image and T.  grad_image f32 [B,C,H,W] and grad_T f32 [B,1,H,W] are the upstream gradients; either may be
 * null (zero; without grad_image no value is read).  Each of the three outputs may be null (not wanted, and then not
 * computed): dL_dfaces_opacity f32 [F], dL_dvalues f32 [N,C] (exact zeros in rows min(n_used[0], N) .. N - 1 and in the row of a
 * slot that does not count), dL_dface_scale f32 [B,F] (needs face_scale).  The formulas are dmr_composite_values_backward's
 * (dmesh_renderer_amd_deferred.h) with values_k = values[row_k]; nothing divides by 1 - o.  With no output wanted the call
 * returns 0 and enqueues nothing. */
int dmr_composite_values_packed_backward(int B, int K, int H, int W, int F, int C, int N, const int32_t* face, const int32_t* row,
                                         const int32_t* n_used, const float* faces_opacity, const float* values,
                                         const float* face_scale, const float* grad_image, const float* grad_T,
                                         float* dL_dfaces_opacity, float* dL_dvalues, float* dL_dface_scale, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DMESH_RENDERER_AMD_PACKED_H */
