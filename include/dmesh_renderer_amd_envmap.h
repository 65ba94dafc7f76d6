/* dmesh_renderer_amd_envmap.h -- direction rows looked up in a learnable lat-long (equirectangular) environment map, as one
 * forward and one backward kernel: the background behind and between the faces (image + T * env(pixel directions)), and, fed a
 * reflected or view direction per packed row, the cheapest specular term of an environment-lit mesh pipeline.
 *
 * A companion of dmesh_renderer_amd.h (same library, libdmesh_renderer_hip.so; errors are read through its
 * dmr_last_error()).  The two calls see rows only: rows in, rows out.
 *
 * THE ENCODING.  d f32 [N,3]; envmap f32 [He,We,C], channel-last like dmesh_renderer_amd_texture.h's texture; y f32 [N,C];
 * 1 <= C <= 16, He, We >= 1.  Per row r:
 *   n = sqrt(d . d) in float32.  The row is SKIPPED when n is not finite or n < 1e-8, or when r >= min(max(n_rows[0], 0), N)
 *       with n_rows i32 [1] on the device (null: N), dmesh_renderer_amd_mlp.h's rule: the count is read on the device.  A
 *       skipped row is not read in grad_out (and past the count not in d): a NaN there reaches nothing; exact zeros in y and
 *       in dL_dd, nothing added to dL_denvmap;
 *   u = d / n, rho2 = ux^2 + uy^2.  The pole axis is z, as in dmesh_renderer_amd_sh.h's table:
 *       theta = acos(clamp(uz, -1, 1)), evaluated as atan2(sqrt(rho2), uz) -- the same angle without acos' loss of digits next to
 *       the poles --,  phi = atan2(uy, ux) -- where rho2 < 1e-12: phi = 0, and the row's dL_dd is an exact 0;
 *   s = phi / (2 pi) + 0.5,  t = theta / pi: row 0 of the map is +z, its last row -z; column 0 starts at phi = -pi (-x, turning
 *       towards -y), +x is the middle of a row;
 *   x = s We - 0.5,  y = t He - 0.5: texel centres sit at half-integers, the texture unit's rule;
 *   x0 = floor(x), fx = x - x0 from the unwrapped coordinate, likewise y0, fy;
 *   columns repeat and rows clamp: (ix0, ix1) = wrap_pair(x0, We, repeat), (iy0, iy1) = wrap_pair(y0, He, clamp)
 *       (csrc/dmr_texture_wrap.hpp) -- the last step before every access, so a NaN, an infinity or 1e30 reads and writes in
 *       bounds (csrc/dmr_envmap_coords.hpp is this whole map from d to (x, y, skipped, pole) and the four indices, plain C++);
 *   y[r] = (1-fy) ((1-fx) envmap[iy0,ix0] + fx envmap[iy0,ix1]) + fy ((1-fx) envmap[iy1,ix0] + fx envmap[iy1,ix1]).
 * In float32 the coordinates carry the rounding of the two atan2 times the map's size: the lookup's deviation from exact
 * arithmetic grows with He and We (README, "Fused environment lookup").
 *
 * THE GRADIENTS.  With g = grad_out[r]:
 *   dL_denvmap = the four bilinear weights times g, summed over the rows: lanes of a wave that hold the same texel merge, the
 *       survivors add into a per-workgroup LDS table of f64 cells keyed by (texel, chunk of four channels), the table leaves as
 *       float atomics when more than half full and at the end, into an output a kernel of this unit has zeroed; what the table
 *       refuses goes out as direct atomics.  So dL_denvmap depends on the order of summation in its last bits;
 *   dL_dd goes through (x, y), (phi, theta) and the normalisation, the cell (the floors) held constant as in the texture unit:
 *       Gx = sum_c g_c dy_c/dx, Gy alike;  gu = (We Gx / (2 pi)) (-uy, ux, 0) / rho2 - (He Gy / pi) (0, 0, 1) / sqrt(rho2);
 *       dL_dd[r] = (gu - u (u . gu)) / n: one plain store per row, no atomics; y and dL_dd do not depend on any order.
 *
 * Out of scope: mip levels and prefiltered roughness (dmesh_renderer_amd_envmap_lod.h looks up a mip pyramid of such a map at a
 * per-row level of detail), cube maps, a map per view, a nearest filter, HDR file reading.
 *
 * Limits: 0 <= N < 2^31, 1 <= C <= DMR_ENVMAP_MAX_CHANNELS, He, We >= 1, He * We * ceil(C / 4) < 2^31.
 *
 * All pointers are device pointers.  Every call only enqueues on `stream`: no host wait, no allocation, safe to capture into a
 * HIP graph.  Every output is fully overwritten; what a kernel adds into (dL_denvmap) is filled first by a kernel of this
 * unit, not by a memset node (dmr_visibility.hip records why).
 * Return value: 0 on success, non-zero on error; dmr_last_error() then returns a description.  The first check that fails
 * decides it, and every check precedes every launch.  The order, for both calls: "bad rows" (N below 0), C, "the map must have
 * at least one texel" (He or We below 1), "map too large", null d (when N > 0), null envmap (when N > 0) -- and only then what a
 * single call asks for: a null output (dmr_envmap_rows, when N > 0), a null grad_out (dmr_envmap_rows_backward, when N > 0).
 */
#ifndef DMESH_RENDERER_AMD_ENVMAP_H
#define DMESH_RENDERER_AMD_ENVMAP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DMR_ENVMAP_MAX_CHANNELS 16
/* Both kernels run at most this many workgroups of 256 rows each and walk further row tiles in a loop. */
#define DMR_ENVMAP_MAX_GROUPS 1024

/* -> y f32 [N,C].  N == 0: returns 0 and enqueues nothing. */
int dmr_envmap_rows(int N, int C, int He, int We, const float* d, const float* envmap, const int32_t* n_rows, float* y, void* stream);

/* The gradients of y.  grad_out f32 [N,C] is the upstream gradient.  Each of the two outputs may be null (not wanted, and then
 * not computed): dL_dd f32 [N,3] and dL_denvmap f32 [He,We,C].  With no output wanted the call returns 0 and enqueues nothing.
 * N == 0: a requested dL_denvmap is written as zeros (one launch), nothing else is enqueued. */
int dmr_envmap_rows_backward(int N, int C, int He, int We, const float* d, const float* envmap, const int32_t* n_rows,
                             const float* grad_out, float* dL_dd, float* dL_denvmap, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DMESH_RENDERER_AMD_ENVMAP_H */
