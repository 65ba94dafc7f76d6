/* dmesh_renderer_amd_sh.h -- the view direction of packed rows as a real spherical-harmonics encoding: the second input of
 * dmesh_renderer_amd_mlp.h's MLP beside dmesh_renderer_amd_hashgrid.h's field, as one forward and one backward kernel, and the
 * map from a packed row to the view it belongs to, which dmesh_renderer_amd_packed.h's rows do not carry.
 *
 * A companion of dmesh_renderer_amd.h (same library, libdmesh_renderer_hip.so; errors are read through its
 * dmr_last_error()).  dmr_packed_row_views reads the packed unit's `row` [B,K,H,W]; the two encoding calls see rows only.
 *
 * THE ENCODING.  x f32 [N,3]; y f32 [N, degree^2], 1 <= degree <= 4.  Per row r:
 *   v = row_view[r] (i32 [N]), or 0 when row_view is null;
 *   w = x[r] - origin[v] with origin f32 [B,3], or w = x[r] when origin is null (the caller hands over directions; B is then
 *       not read and v is 0);
 *   n = sqrt(w . w), d = w / n -- and d = (0, 0, 0) when n is not finite or n < 1e-8: the row's dL/dx is then an exact 0 and it
 *       adds nothing to dL/dorigin;
 *   y[r, l*l + l + m] = Y_lm(d), the real spherical harmonics in the Condon-Shortley sign convention (tiny-cuda-nn's
 *       "SphericalHarmonics", the Gaussian-splatting code's basis), as homogeneous polynomials of d = (x, y, z):
 *          0   0.28209479177387814
 *          1  -0.4886025119029199 y            2   0.4886025119029199 z             3  -0.4886025119029199 x
 *          4   1.0925484305920792 xy           5  -1.0925484305920792 yz            6   0.31539156525252005 (2zz - xx - yy)
 *          7  -1.0925484305920792 xz           8   0.5462742152960396 (xx - yy)
 *          9  -0.5900435899266435 y(3xx - yy)  10  2.890611442640554 xyz            11 -0.4570457994644658 y(4zz - xx - yy)
 *          12  0.3731763325901154 z(2zz - 3xx - 3yy)                                13 -0.4570457994644658 x(4zz - xx - yy)
 *          14  1.445305721320277 z(xx - yy)    15 -0.5900435899266435 x(xx - 3yy)
 * A row is SKIPPED -- not read, in x and in grad_out: a NaN there reaches nothing; exact zeros in y and in dL_dx, nothing added
 * to dL_dorigin -- when v lies outside [0, B) (a row_view of -1 is what dmr_packed_row_views gives a row no slot owns), or when
 * r >= min(max(n_rows[0], 0), N) with n_rows i32 [1] on the device (null: N), dmesh_renderer_amd_mlp.h's rule: the count is
 * read on the device.  A row that is read and has d = 0 gives y = (0.2820..., 0, ..., 0).
 *
 * THE GRADIENTS.  With g = grad_out[r] and gd = sum_i g_i dY_i/dd (the free-vector derivative of the polynomials):
 *   dL/dw = (gd - d (d . gd)) / n,   dL_dx[r] = dL/dw (a plain store per row),   dL_dorigin[v] = - sum over the rows of v of dL/dw.
 * The projection makes the result independent of the polynomials' form off the sphere.  dL_dorigin sums on chip: a wave whose
 * rows are of one view (rows are numbered view-major, so almost every wave) reduces its three values across lanes and adds
 * once into a per-workgroup LDS table of f64 cells [B][3], a mixed wave adds per lane; the table leaves once per workgroup,
 * with one global float add per non-zero cell, into an output a kernel of this unit has zeroed.  So dL_dorigin depends on the
 * order of summation in its last bits; y and dL_dx do not.
 *
 * Limits: 0 <= N < 2^31, 1 <= degree <= 4, 1 <= B <= DMR_SH_MAX_VIEWS when origin is given.
 *
 * All pointers are device pointers.  Every call only enqueues on `stream`: no host wait, no allocation, safe to capture into a
 * HIP graph.  Every output is fully overwritten; what a kernel adds into (dL_dorigin) or writes sparsely (view_out) is filled
 * first by a kernel of this unit, not by a memset node (dmr_visibility.hip records why).
 * Return value: 0 on success, non-zero on error; dmr_last_error() then returns a description.  The first check that fails
 * decides it, and every check precedes every launch.  The order, for the two encoding calls: "bad rows" (N below 0), degree,
 * row_view without origin, B (when origin is given), null x (when N > 0) -- and only then what a single call asks for: a null
 * output (dmr_sh_rows, when N > 0), a null grad_out (dmr_sh_rows_backward, when N > 0), dL_dorigin without origin.
 * For dmr_packed_row_views: "bad dimensions" (B, H, W or N below 0), K outside 1..32, "problem too large" (B K H W or the
 * launch grid at or past 2^31), null row (when B H W > 0), null output (when N > 0).
 */
#ifndef DMESH_RENDERER_AMD_SH_H
#define DMESH_RENDERER_AMD_SH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DMR_SH_MAX_DEGREE 4
#define DMR_SH_MAX_VIEWS 1024
/* Both encoding kernels run at most this many workgroups of 256 rows each and walk further row tiles in a loop. */
#define DMR_SH_MAX_GROUPS 1024

/* -> view_out i32 [N]: entry r is the view b of the slot that owns row r -- a slot (b, k, y, x) of row i32 [B,K,H,W] counts
 * when 0 <= row < N --, -1 in every row no slot owns (the tail [min(n_used, N), N) under a capacity).  Two slots claiming one
 * row (a `row` made for other lists): one of their views, in bounds.  Two launches: the fill with -1, then one walk of the
 * slots, 64 pixels of an image row per wave, 4 bytes written per counting slot.  N == 0 or B H W == 0: returns 0 and enqueues
 * nothing (view_out is not touched). */
int dmr_packed_row_views(int B, int K, int H, int W, int N, const int32_t* row, int32_t* view_out, void* stream);

/* -> y f32 [N, degree^2].  N == 0: returns 0 and enqueues nothing. */
int dmr_sh_rows(int N, int degree, int B, const float* x, const float* origin, const int32_t* row_view, const int32_t* n_rows,
                float* y, void* stream);

/* The gradients of y.  grad_out f32 [N, degree^2] is the upstream gradient.  Each of the two outputs may be null (not wanted,
 * and then not computed): dL_dx f32 [N,3] and dL_dorigin f32 [B,3] (needs origin).  With no output wanted the call returns 0
 * and enqueues nothing.  N == 0: a requested dL_dorigin is written as zeros (one launch), nothing else is enqueued. */
int dmr_sh_rows_backward(int N, int degree, int B, const float* x, const float* origin, const int32_t* row_view,
                         const int32_t* n_rows, const float* grad_out, float* dL_dx, float* dL_dorigin, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DMESH_RENDERER_AMD_SH_H */
