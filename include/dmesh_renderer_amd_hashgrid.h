/* dmesh_renderer_amd_hashgrid.h -- a multiresolution hash-grid encoding of packed rows of 3-D points: the learned field in front
 * of dmesh_renderer_amd_mlp.h's MLP, as one forward and one backward kernel.
 *
 * A companion of dmesh_renderer_amd.h (same library, libdmesh_renderer_hip.so; errors are read through its
 * dmr_last_error()).  No dmr_scene and no fragment lists: the calls see rows only.
 *
 * The grid has L levels of F features over the unit cube.  Level l has resolution R_l = resolutions[l] (R_l cells, R_l + 1 grid
 * vertices per axis) and owns the rows [offsets[l], offsets[l+1]) of `table` f32 [offsets[L], F].  With T = 2^log2_T a level is
 *   DENSE   when (R_l + 1)^3 <= T:  (R_l + 1)^3 rows, grid vertex (ix, iy, iz) in row ix + (R_l + 1) (iy + (R_l + 1) iz);
 *   HASHED  otherwise:              T rows, the vertex in row ((ix * 1) ^ (iy * 2654435761) ^ (iz * 805459861)) & (T - 1), the
 *                                   products taken modulo 2^32.
 * dmr_hashgrid_layout states that rule; both calls derive the layout from (L, log2_T, resolutions) through it.
 * Limits: 1 <= L <= 16, F in {1, 2, 4, 8}, L * F <= 64 (the MLP's Cin), 4 <= log2_T <= 24, 1 <= R_l <= 65536, 0 <= N < 2^31.
 *
 * x f32 [N,3]; y f32 [N, L*F], level-major channels.  For each coordinate u of a row and each level:
 *   u_c = clamp(u, 0, 1) with NaN counting as 0;  p = u_c R_l;  i = min(floor(p), R_l - 1);  t = p - i in [0, 1]
 * and y[r, l F + f] = sum over the 8 corners c of w_c table[offsets[l] + row(i + c), f], w_c the trilinear weight from
 * (t_x, t_y, t_z).  The cell and the hash are constants of the gradients; dL/dx of a coordinate that is NaN or outside [0, 1]
 * is exactly 0, at exactly 0 and 1 it passes.  Every row index is clamped (dense) or masked (hashed) into its level's slice as
 * the last step before the access: a NaN, an Inf or 1e30 in x reads and writes in bounds.  Offsets into y, grad_out and table
 * are 64-bit.
 *
 * n_rows i32 [1] on the device, or null (= N): rows r >= min(max(n_rows[0], 0), N) are NOT READ, in x and in grad_out; they get
 * exact zeros in y and in dL_dx and add nothing to dL_dtable.  The count is read on the device.
 *
 * `resolutions` is a HOST array of L int32 (it is read during the call, not later); every other pointer is a device pointer.
 * Both calls only enqueue on `stream`: no host wait, no allocation, safe to capture into a HIP graph.  Every output is fully
 * overwritten; dL_dtable, which the backward adds into, is zeroed first by a kernel of this unit (not by a memset node).
 * Return value: 0 on success, non-zero on error; dmr_last_error() then returns a description.  The first check that fails
 * decides it, in this order: "bad rows" (N below 0), L, F, L * F, log2_T, null resolutions, a resolution outside 1..65536, null
 * x (when N > 0), null table -- and only then what a single call asks for: a null output (when N > 0), a null grad_out (when
 * N > 0).
 */
#ifndef DMESH_RENDERER_AMD_HASHGRID_H
#define DMESH_RENDERER_AMD_HASHGRID_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DMR_HASHGRID_MAX_LEVELS 16
#define DMR_HASHGRID_MAX_CHANNELS 64
/* Both kernels run at most this many workgroups of 256 rows each and walk further row tiles in a loop. */
#define DMR_HASHGRID_MAX_GROUPS 1024

/* Host only: offsets_out[0 .. L] = the running sums of the levels' row counts by the rule above (offsets_out[L] = the rows of
 * `table`).  Checks L, log2_T, null resolutions, the resolutions, null offsets_out, in this order. */
int dmr_hashgrid_layout(int L, int log2_T, const int32_t* resolutions, int64_t* offsets_out);

/* -> y f32 [N, L*F].  N == 0: returns 0 and enqueues nothing. */
int dmr_hashgrid_rows(int N, int L, int F, int log2_T, const int32_t* resolutions, const float* x, const float* table,
                      const int32_t* n_rows, float* y, void* stream);

/* The gradients of y.  grad_out f32 [N, L*F] is the upstream gradient.  Each of the two outputs may be null (not wanted, and
 * then not computed): dL_dx f32 [N,3] (a plain store per row; needs no atomics) and dL_dtable f32 [offsets[L], F] (zeroed, then
 * added into: sums of a wave's lanes and of a workgroup's rows are formed on chip first; reads no table).  With no output
 * wanted the call returns 0 and enqueues nothing.  N == 0: a requested dL_dtable is written as zeros (one launch), nothing else
 * is enqueued. */
int dmr_hashgrid_rows_backward(int N, int L, int F, int log2_T, const int32_t* resolutions, const float* x, const float* table,
                               const int32_t* n_rows, const float* grad_out, float* dL_dx, float* dL_dtable, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DMESH_RENDERER_AMD_HASHGRID_H */
