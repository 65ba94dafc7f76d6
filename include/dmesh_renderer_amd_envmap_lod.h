/* dmesh_renderer_amd_envmap_lod.h -- a mip pyramid of a learnable lat-long (equirectangular) environment map, built on the
 * device, and direction rows looked up in it at a per-row level of detail: the specular term of a rough surface (a mirrored view
 * ray per packed row, a roughness per row mapped to a level by the caller), next to dmesh_renderer_amd_envmap.h's single tap,
 * which makes every surface a perfect mirror.  Two pairs of calls: the builder and its backward, the lookup and its backward.
 *
 * A companion of dmesh_renderer_amd.h (same library, libdmesh_renderer_hip.so; errors are read through its
 * dmr_last_error()).  The calls see rows and maps only.
 *
 * THE LAYOUT.  The spec is (He, We, L), 1 <= L <= DMR_ENVMAP_LOD_MAX_LEVELS.  Level l has He_l = He >> l rows and We_l = We >> l
 * columns; He and We must be multiples of 2^(L-1) (12 x 20 with L = 3 is allowed).  pyramid is f32 [T,C], channel-last,
 * T = sum_l He_l We_l: level l is the row-major [He_l, We_l, C] block that starts at row off_l = sum_{j<l} He_j We_j; level 0 is
 * the base map itself.  1 <= C <= 16, T * ceil(C / 4) < 2^31.
 *
 * THE BUILDER.  dmr_envmap_pyramid copies envmap [He,We,C] into level 0 and forms level l+1 at (i, j) as
 *       ((a + b) + (c + d)) * 0.25,   a, b = level l at (2i, 2j), (2i, 2j+1);  c, d = the same columns of row 2i+1
 * -- this order of summation is part of the contract --, one small launch per level, stream-ordered.  It is a BOX mip chain in
 * the map's own parameterisation, NOT a solid-angle or GGX prefilter: the lookup below accepts any [T,C] tensor in this layout,
 * so a caller may pass a pyramid prefiltered elsewhere.  dmr_envmap_pyramid_backward is one gather launch without atomics: per
 * base texel (y, x) Horner from the coarsest level down, acc = g_l[y >> l, x >> l] + 0.25 * acc, -> dL_denvmap [He,We,C].
 * Multiplying by 0.25 is exact: both directions equal float32 evaluation of these formulas bit for bit on finite, normal values.
 *
 * THE ENCODING of the lookup.  d f32 [N,3]; lod f32, one per row, lod_stride >= 1 floats apart (a column of a wider tensor needs
 * no copy); y f32 [N,C].  Per row r:
 *   n, u, rho2, theta, phi, s, t exactly as dmesh_renderer_amd_envmap.h states them: theta = atan2(sqrt(rho2), uz), the pole rule
 *       rho2 < 1e-12 (phi = 0, an exact 0 in dL_dd), and the SKIPPED row (n not finite or below 1e-8, or r >= min(max(n_rows[0], 0), N)
 *       with n_rows i32 [1] on the device, null: N).  A skipped row reads neither lod nor grad_out (past the count not d either): exact
 *       zeros in y, dL_dd and dL_dlod, nothing added to dL_dpyramid;
 *   lam = lod >= 0 ? (lod <= L-1 ? lod : L-1) : 0 -- a NaN compares false and becomes 0, +Inf becomes L-1;
 *       inside = lod > 0 && lod < L-1;  l0 = min(floor(lam), L-2), l1 = l0 + 1, f = lam - l0 in [0, 1];  L == 1: l0 = l1 = 0, f = 0,
 *       inside false;
 *   B_l = the bilinear mix of dmesh_renderer_amd_envmap.h at level l, with that level's own x = s We_l - 0.5, y = t He_l - 0.5, its
 *       own floors and fractions, columns repeating and rows clamped on (We_l, He_l) -- wrap_pair is the last step before every
 *       access, and both levels are clamped into [0, L-1] (csrc/dmr_envmap_lod_coords.hpp: env_angles, env_place, env_lod_levels,
 *       plain C++);
 *   y[r] = (1-f) B_l0 + f B_l1.  A level whose weight is exactly 0 is not read by the forward: a non-finite texel there is
 *       unspecified.
 * The two atan2, the square root and the normalisation are evaluated once per row; the eight addresses and weights come from
 * (s, t) per level.
 *
 * THE GRADIENTS.  With g = grad_out[r]:
 *   dL_dlod[r] = (B_l1 - B_l0) . g where inside holds, an exact 0 elsewhere; at an integer lod this is the derivative to the right
 *       (l1 is read there when dL_dlod is wanted, and for dL_dlod alone: what it holds reaches neither dL_dd nor dL_dpyramid).  A
 *       plain store per row into a contiguous f32 [N];
 *   dL_dd holds the cell constant at both levels: Gphi = sum_l w_l (We_l / 2 pi) Gx_l, Gtheta = sum_l w_l (He_l / pi) Gy_l with
 *       w = (1-f, f) and Gx_l, Gy_l the derivatives of B_l . g by its x and y; then gu = Gphi (-uy, ux, 0) / rho2 - Gtheta (0, 0, 1) /
 *       sqrt(rho2) and dL_dd[r] = (gu - u (u . gu)) / n; an exact 0 at a pole.  A plain store per row;
 *   dL_dpyramid [T,C] = the eight weights (level weight times bilinear weight) times g, summed over the rows: lanes of a wave that
 *       hold the same (texel, chunk of four channels) merge, the survivors add into a per-workgroup LDS table of f64 cells keyed by
 *       (off_l + iy We_l + ix) * ceil(C / 4) + chunk, the table leaves as float atomics when more than half full and at the end,
 *       into an output a kernel of this unit has zeroed; what the table refuses goes out as direct atomics.  So dL_dpyramid
 *       depends on the order of summation in its last bits; y, dL_dd and dL_dlod do not.
 *
 * Out of scope: a GGX or solid-angle prefilter, cube maps, a map per view, anisotropic footprints, a level of detail from
 * screen-space derivatives.
 *
 * Limits: 0 <= N < 2^31, 1 <= C <= DMR_ENVMAP_LOD_MAX_CHANNELS, 1 <= L <= DMR_ENVMAP_LOD_MAX_LEVELS, He and We positive multiples
 * of 2^(L-1), T * ceil(C / 4) < 2^31, lod_stride >= 1.
 *
 * All pointers are device pointers.  Every call only enqueues on `stream`: no host wait, no allocation, safe to capture into a
 * HIP graph.  Every output is fully overwritten; what a kernel adds into (dL_dpyramid) is filled first by a kernel of this
 * unit, not by a memset node.
 * Return value: 0 on success, non-zero on error; dmr_last_error() then returns a description.  The first check that fails
 * decides it, and every check precedes every launch.  The order: "bad rows" (N below 0; the lookup's two calls only), C, L, "the
 * map must have at least one texel" (He or We below 1), "He and We must be multiples of 2^(L-1)", "pyramid too large" -- then, for
 * the lookup's two calls: "lod_stride must be at least 1", null d, null lod, null pyramid (each when N > 0), and only then what a
 * single call asks for: a null output (dmr_envmap_lod_rows, when N > 0), a null grad_out (dmr_envmap_lod_rows_backward, when
 * N > 0); for the builder's two calls: a null envmap, then a null output (dmr_envmap_pyramid); a null grad_pyramid, then a null
 * output (dmr_envmap_pyramid_backward).
 */
#ifndef DMESH_RENDERER_AMD_ENVMAP_LOD_H
#define DMESH_RENDERER_AMD_ENVMAP_LOD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DMR_ENVMAP_LOD_MAX_CHANNELS 16
#define DMR_ENVMAP_LOD_MAX_LEVELS 12
/* The lookup's kernels run at most this many workgroups of 256 rows each and walk further row tiles in a loop. */
#define DMR_ENVMAP_LOD_MAX_GROUPS 1024

/* envmap f32 [He,We,C] -> pyramid f32 [T,C]: L launches. */
int dmr_envmap_pyramid(int C, int He, int We, int L, const float* envmap, float* pyramid, void* stream);

/* grad_pyramid f32 [T,C] -> dL_denvmap f32 [He,We,C]: one launch. */
int dmr_envmap_pyramid_backward(int C, int He, int We, int L, const float* grad_pyramid, float* dL_denvmap, void* stream);

/* -> y f32 [N,C].  N == 0: returns 0 and enqueues nothing. */
int dmr_envmap_lod_rows(int N, int C, int He, int We, int L, int lod_stride, const float* d, const float* lod, const float* pyramid,
                        const int32_t* n_rows, float* y, void* stream);

/* The gradients of y.  grad_out f32 [N,C] is the upstream gradient.  Each of the three outputs may be null (not wanted, and then
 * not computed): dL_dd f32 [N,3], dL_dlod f32 [N] and dL_dpyramid f32 [T,C].  With no output wanted the call returns 0 and
 * enqueues nothing.  N == 0: a requested dL_dpyramid is written as zeros (one launch), nothing else is enqueued. */
int dmr_envmap_lod_rows_backward(int N, int C, int He, int We, int L, int lod_stride, const float* d, const float* lod,
                                 const float* pyramid, const int32_t* n_rows, const float* grad_out, float* dL_dd, float* dL_dlod,
                                 float* dL_dpyramid, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DMESH_RENDERER_AMD_ENVMAP_LOD_H */
