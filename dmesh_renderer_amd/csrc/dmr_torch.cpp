// dmr_torch.cpp -- `dmesh_renderer_amd._C`: the binding surface of the reference extension (ext.cpp:4-11) as a
// compiled PyTorch-ROCm module over the C ABI of libdmesh_renderer_hip.so (include/dmesh_renderer_amd.h).
//
//     render_tris            <- RasterizeTrianglesCUDA          (render.cu:29-132)
//     render_tris_backward   <- RasterizeTrianglesBackwardCUDA  (render.cu:134-208)
//     render_tets            <- RenderFTetsCUDA                 (render.cu:213-336)
//     render_tets_backward   <- RenderFTetsBackwardCUDA         (render.cu:338-412)
//
// Same positional arguments, tuple arity, dtypes / shapes and error behaviour (RuntimeError with the reference's
// messages, render.cu:49-79,237-277).  This file is what render.cu is in the reference: shape checks, output and
// scratch allocation (PyTorch's caching allocator: no device allocation in the steady state, and the graph-private
// pool under torch.cuda.graph capture), the current stream, raw-pointer hand-off.  It holds no compute and no HIP
// kernel; the C ABI library is loaded with dlopen (DMR_LIBRARY=<path> selects another build of it, e.g. the ablation
// build of build.py --ablation) and nothing here works without it: there is no fallback of any kind.
//
// Extensions over the reference (keyword arguments, all optional):
//   rows=(begin, end)        a band of 16-pixel tile rows (multi-GPU tile-row sharding); (0, 0) = everything
//   fill_outside=True        render_tris: zero the pixels outside the band (False: leave them uninitialised)
//   flat_out=None            backward: one caller-owned fp32 buffer receiving the gradients back to back (the payload
//                            of the one all-reduce in sharding.py); the returned tensors are views into it
//   full_grads=False         render_tets_backward: also dL_dverts and dL_dfaces_intense (DMR_FLAG_TET_FULL_GRADS, beyond
//                            the reference) -> (dL_dverts, dL_dverts_color, dL_dfaces_opacity, dL_dfaces_intense)
//   exact_grads=False        render_tris_backward: dL_dverts is the exact derivative of the image (DMR_FLAG_TRI_EXACT_GRADS)
//   camera_grads=False       render_tris_backward: also dL_dinv_mv_mats, dL_dinv_proj_mats [B,4,4] (DMR_FLAG_TRI_CAMERA_GRADS,
//                            implies exact_grads) -> the five gradients, then those two
//                            render_tets_backward: also dL_dinv_mv_mats, dL_dinv_proj_mats, dL_dmv_mats, dL_dproj_mats
//                            [B,4,4] (DMR_FLAG_TET_CAMERA_GRADS, implies full_grads) -> the four full gradients, then those
//   fragment_grads=None      render_tris_backward: (pix_to_face i32 [B,K,H,W], grad_bary f32 [B,K,2,H,W]), 1 <= K <= 32: the gradient
//                            of the fragment lists' barycentrics joins dL_dverts (and, with camera_grads, the matrices' gradients):
//                            DMR_FLAG_TRI_FRAGMENT_GRADS; the tuple is the level's, unchanged
//                            render_tets_backward: the same two tensors for the tet fragment lists' unclamped barycentrics
//                            (DMR_FLAG_TET_FRAGMENT_GRADS); raises the level to at least full_grads, whose tuple is unchanged
//   fragments=0              render_tris: K > 0 (at most 32): per-pixel fragment lists (DMR_FLAG_TRI_FRAGMENTS) -> the tuple gains
//                            face i32 [B,K,H,W], bary f32 [B,K,2,H,W], count i32 [B,H,W] behind the four scratch tensors
//                            render_tets: the same (DMR_FLAG_TET_FRAGMENTS): the faces of the march, in march order
//   composite_fragments(face, bary, faces, faces_opacity, vert_attrs, face_scale=None) -> (image [B,C,H,W], T [B,1,H,W]) and
//   composite_fragments_backward(..., grad_image, grad_T, need=(opacity, attrs, scale, bary)) -> those four gradients or None:
//                            fragments.composite_fused, over include/dmesh_renderer_amd_shade.h (SUPPORTS_FRAGMENT_COMPOSITE)
//   composite_texture(face, bary, uv_faces, faces_opacity, vert_uvs, texture, face_scale=None, wrap=0) -> (image, T) and
//   composite_texture_backward(..., grad_image, grad_T, need=(opacity, uvs, texture, scale, bary)) -> those five gradients or None:
//                            fragments.composite_texture_fused, over include/dmesh_renderer_amd_texture.h (SUPPORTS_FRAGMENT_TEXTURE)
//   face_visibility(face, faces_opacity, pixel_weight=None, coverage=False) -> (vis [B,F], max_weight [B,F] | None, pixels i32 [B,F] | None) and
//   face_visibility_backward(face, faces_opacity, pixel_weight, grad_vis, need=(opacity, pixel_weight)) -> those two gradients or None:
//                            fragments.face_visibility_fused, over include/dmesh_renderer_amd_visibility.h (SUPPORTS_FRAGMENT_VISIBILITY)
//   interpolate_fragments(face, bary, faces, vert_attrs) -> out [B,K,C,H,W] and
//   interpolate_fragments_backward(..., grad_out, need=(attrs, bary)) -> those two gradients or None; composite_values(face,
//   faces_opacity, values, face_scale=None) -> (image, T) and composite_values_backward(..., grad_image, grad_T,
//   need=(opacity, values, scale)) -> those three or None: fragments.interpolate_fused / composite_values_fused, over
//                            include/dmesh_renderer_amd_deferred.h (SUPPORTS_FRAGMENT_DEFERRED)
//   pack_slots(face, F, capacity) -> (row [B,K,H,W] int32, n_used [1] int32); interpolate_packed(face, bary, row, n_used, faces,
//   vert_attrs, N) -> out [N,C] and interpolate_packed_backward(..., grad_out, need=(attrs, bary)); composite_values_packed(face,
//   row, faces_opacity, values [N,C], face_scale=None) -> (image, T) and composite_values_packed_backward(face, row, n_used, ...,
//   grad_image, grad_T, need=(opacity, values, scale)): the packed, channel-last form of the four above
//   (fragments.pack_slots_fused / interpolate_packed_fused / composite_values_packed_fused), over
//                            include/dmesh_renderer_amd_packed.h (SUPPORTS_FRAGMENT_PACKED)
//   mlp_rows(x [N,Cin], weights, biases, act, oact, n_rows=None) -> y [N,Cout] and mlp_rows_backward(..., grad_out, need_x,
//   need_w, need_b) -> (dL_dx | None, [dL_dW_l | None], [dL_db_l | None]): a 1- or 2-hidden-layer MLP over packed rows
//   (fragments.mlp_rows_fused), over include/dmesh_renderer_amd_mlp.h (SUPPORTS_FRAGMENT_MLP)
//   hashgrid_rows(x [N,3], table [rows,F], resolutions, log2_T, n_rows=None) -> y [N,L*F] and hashgrid_rows_backward(...,
//   grad_out, need_x, need_table) -> (dL_dx | None, dL_dtable | None): a multiresolution hash-grid encoding of packed rows
//   (fragments.hashgrid_rows_fused), over include/dmesh_renderer_amd_hashgrid.h (SUPPORTS_FRAGMENT_HASHGRID)
//   packed_row_views(row [B,K,H,W], rows) -> view i32 [rows], sh_rows(x [N,3], degree, origin=None, row_view=None, n_rows=None)
//   -> y [N,degree^2] and sh_rows_backward(..., grad_out, need_x, need_origin) -> (dL_dx | None, dL_dorigin | None): the view
//   direction of packed rows as spherical harmonics (fragments.packed_row_views_fused, sh_rows_fused), over
//   include/dmesh_renderer_amd_sh.h (SUPPORTS_FRAGMENT_SH)
//   envmap_rows(d [N,3], envmap [He,We,C], n_rows=None) -> y [N,C] and envmap_rows_backward(..., grad_out, need_d, need_envmap)
//   -> (dL_dd | None, dL_denvmap | None): direction rows looked up in a lat-long environment map (fragments.envmap_rows_fused),
//   over include/dmesh_renderer_amd_envmap.h (SUPPORTS_FRAGMENT_ENVMAP)
//   envmap_pyramid(envmap [He,We,C], levels) -> pyramid [T,C] and envmap_pyramid_backward(grad_pyramid, He, We, levels) -> dL_denvmap:
//   the mip pyramid of a lat-long map (fragments.envmap_pyramid_fused); envmap_lod_rows(d [N,3], lod [N] or [N,1] (any stride >= 1),
//   pyramid [T,C], He, We, levels, n_rows=None) -> y [N,C] and envmap_lod_rows_backward(..., grad_out, need_d, need_lod, need_pyramid)
//   -> (dL_dd | None, dL_dlod | None, dL_dpyramid | None): direction rows looked up in it at a per-row level of detail
//   (fragments.envmap_lod_rows_fused), over include/dmesh_renderer_amd_envmap_lod.h (SUPPORTS_FRAGMENT_ENVMAP_LOD)
//   surface_packed(face, bary, row, n_used, faces, verts [P,3], origin [B,3], N) -> (hit, normal, reflect) [N,3] and
//   surface_packed_backward(..., grad_hit, grad_normal, grad_reflect (None = zero), need=(verts, bary, origin)) -> those three
//   gradients or None: the surface frame of packed rows (fragments.surface_packed_fused), over
//   include/dmesh_renderer_amd_surface.h (SUPPORTS_FRAGMENT_SURFACE)
//   set_async(True)          calls never wait for the device (DMR_FLAG_ASYNC; automatic under stream capture):
//                            `num_rendered` is then the capacity used, overflowed() reports a scene that outgrew it
#include <torch/extension.h>

#include <c10/core/DeviceGuard.h>
#include <c10/hip/HIPStream.h>
#include <dlfcn.h>

#include <array>
#include <atomic>
#include <cstdlib>
#include <optional>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../include/dmesh_renderer_amd.h"
#include "../../include/dmesh_renderer_amd_shade.h"
#include "../../include/dmesh_renderer_amd_texture.h"
#include "../../include/dmesh_renderer_amd_visibility.h"
#include "../../include/dmesh_renderer_amd_deferred.h"
#include "../../include/dmesh_renderer_amd_packed.h"
#include "../../include/dmesh_renderer_amd_mlp.h"
#include "../../include/dmesh_renderer_amd_hashgrid.h"
#include "../../include/dmesh_renderer_amd_sh.h"
#include "../../include/dmesh_renderer_amd_envmap.h"
#include "../../include/dmesh_renderer_amd_envmap_lod.h"
#include "../../include/dmesh_renderer_amd_surface.h"

namespace {

constexpr int NUM_CHANNELS = 3;  // cuda_*/config.h:4

[[noreturn]] void err(const std::string& m) { throw std::runtime_error(m); }

// ---- the C ABI, bound at import ---------------------------------------------------------------------------------
struct Abi {
    void* handle = nullptr;
    std::string path;
    decltype(&dmr_tri_forward) tri_forward = nullptr;
    decltype(&dmr_tri_backward) tri_backward = nullptr;
    decltype(&dmr_tet_forward) tet_forward = nullptr;
    decltype(&dmr_tet_backward) tet_backward = nullptr;
    decltype(&dmr_invert_mats) invert_mats = nullptr;
    decltype(&dmr_export) export_item = nullptr;
    decltype(&dmr_profile_enable) profile_enable = nullptr;
    decltype(&dmr_profile_collect) profile_collect = nullptr;
    decltype(&dmr_stage_name) stage_name = nullptr;
    decltype(&dmr_last_error) last_error = nullptr;
    decltype(&dmr_overflowed) overflowed = nullptr;
    decltype(&dmr_redo_count) redo_count = nullptr;
    decltype(&dmr_abi_version) abi_version = nullptr;
    decltype(&dmr_build_arch) build_arch = nullptr;
    // dmesh_renderer_amd_shade.h: optional (SUPPORTS_FRAGMENT_COMPOSITE), a library without them still loads
    decltype(&dmr_composite_fragments) composite_fragments = nullptr;
    decltype(&dmr_composite_fragments_backward) composite_fragments_backward = nullptr;
    // dmesh_renderer_amd_texture.h: optional too (SUPPORTS_FRAGMENT_TEXTURE)
    decltype(&dmr_composite_texture) composite_texture = nullptr;
    decltype(&dmr_composite_texture_backward) composite_texture_backward = nullptr;
    // dmesh_renderer_amd_visibility.h: optional too (SUPPORTS_FRAGMENT_VISIBILITY)
    decltype(&dmr_face_visibility) face_visibility = nullptr;
    decltype(&dmr_face_visibility_backward) face_visibility_backward = nullptr;
    // dmesh_renderer_amd_deferred.h: optional too (SUPPORTS_FRAGMENT_DEFERRED), all four or none
    decltype(&dmr_interpolate_fragments) interpolate_fragments = nullptr;
    decltype(&dmr_interpolate_fragments_backward) interpolate_fragments_backward = nullptr;
    decltype(&dmr_composite_values) composite_values = nullptr;
    decltype(&dmr_composite_values_backward) composite_values_backward = nullptr;
    // dmesh_renderer_amd_packed.h: optional too (SUPPORTS_FRAGMENT_PACKED), all five or none
    decltype(&dmr_pack_slots) pack_slots = nullptr;
    decltype(&dmr_interpolate_packed) interpolate_packed = nullptr;
    decltype(&dmr_interpolate_packed_backward) interpolate_packed_backward = nullptr;
    decltype(&dmr_composite_values_packed) composite_values_packed = nullptr;
    decltype(&dmr_composite_values_packed_backward) composite_values_packed_backward = nullptr;
    // dmesh_renderer_amd_mlp.h: optional too (SUPPORTS_FRAGMENT_MLP), both or none
    decltype(&dmr_mlp_rows) mlp_rows = nullptr;
    decltype(&dmr_mlp_rows_backward) mlp_rows_backward = nullptr;
    // dmesh_renderer_amd_hashgrid.h: optional too (SUPPORTS_FRAGMENT_HASHGRID), all three or none
    decltype(&dmr_hashgrid_layout) hashgrid_layout = nullptr;
    decltype(&dmr_hashgrid_rows) hashgrid_rows = nullptr;
    decltype(&dmr_hashgrid_rows_backward) hashgrid_rows_backward = nullptr;
    // dmesh_renderer_amd_sh.h: optional too (SUPPORTS_FRAGMENT_SH), all three or none
    decltype(&dmr_packed_row_views) packed_row_views = nullptr;
    decltype(&dmr_sh_rows) sh_rows = nullptr;
    decltype(&dmr_sh_rows_backward) sh_rows_backward = nullptr;
    // dmesh_renderer_amd_envmap.h: optional too (SUPPORTS_FRAGMENT_ENVMAP), both or none
    decltype(&dmr_envmap_rows) envmap_rows = nullptr;
    decltype(&dmr_envmap_rows_backward) envmap_rows_backward = nullptr;
    // dmesh_renderer_amd_envmap_lod.h: optional too (SUPPORTS_FRAGMENT_ENVMAP_LOD), all four or none
    decltype(&dmr_envmap_pyramid) envmap_pyramid = nullptr;
    decltype(&dmr_envmap_pyramid_backward) envmap_pyramid_backward = nullptr;
    decltype(&dmr_envmap_lod_rows) envmap_lod_rows = nullptr;
    decltype(&dmr_envmap_lod_rows_backward) envmap_lod_rows_backward = nullptr;
    // dmesh_renderer_amd_surface.h: optional too (SUPPORTS_FRAGMENT_SURFACE), both or none
    decltype(&dmr_surface_packed) surface_packed = nullptr;
    decltype(&dmr_surface_packed_backward) surface_packed_backward = nullptr;
};

Abi g_abi;
std::atomic<int> g_async{0};

template <class F>
void bind(F& fn, const char* name) {
    void* p = dlsym(g_abi.handle, name);
    if (!p) throw std::runtime_error(g_abi.path + " does not export " + name);
    fn = reinterpret_cast<F>(p);
}

void load_abi() {
    const char* env = std::getenv("DMR_LIBRARY");
    std::string path;
    if (env && *env) path = env;
    else {
        Dl_info info;
        if (!dladdr(reinterpret_cast<void*>(&load_abi), &info) || !info.dli_fname)
            throw std::runtime_error("cannot locate the dmesh_renderer_amd package directory");
        path = info.dli_fname;
        const size_t slash = path.find_last_of('/');
        path = (slash == std::string::npos ? std::string(".") : path.substr(0, slash)) + "/libdmesh_renderer_hip.so";
    }
    g_abi.path = path;
    g_abi.handle = dlopen(path.c_str(), RTLD_NOW | RTLD_LOCAL);
    if (!g_abi.handle) {
        const char* why = dlerror();  // (a second call would return NULL: the message is consumed by the first)
        throw std::runtime_error(path + " cannot be loaded (" + std::string(why ? why : "?") +
                                 "): the HIP library is not built (run `python -m dmesh_renderer_amd.build`); there is no CPU fallback");
    }
    bind(g_abi.tri_forward, "dmr_tri_forward"); bind(g_abi.tri_backward, "dmr_tri_backward");
    bind(g_abi.tet_forward, "dmr_tet_forward"); bind(g_abi.tet_backward, "dmr_tet_backward");
    bind(g_abi.invert_mats, "dmr_invert_mats"); bind(g_abi.export_item, "dmr_export");
    bind(g_abi.profile_enable, "dmr_profile_enable"); bind(g_abi.profile_collect, "dmr_profile_collect");
    bind(g_abi.stage_name, "dmr_stage_name"); bind(g_abi.last_error, "dmr_last_error");
    bind(g_abi.overflowed, "dmr_overflowed"); bind(g_abi.redo_count, "dmr_redo_count"); bind(g_abi.abi_version, "dmr_abi_version");
    bind(g_abi.build_arch, "dmr_build_arch");
    g_abi.composite_fragments = reinterpret_cast<decltype(g_abi.composite_fragments)>(dlsym(g_abi.handle, "dmr_composite_fragments"));
    g_abi.composite_fragments_backward =
        reinterpret_cast<decltype(g_abi.composite_fragments_backward)>(dlsym(g_abi.handle, "dmr_composite_fragments_backward"));
    if (!g_abi.composite_fragments || !g_abi.composite_fragments_backward) g_abi.composite_fragments = nullptr, g_abi.composite_fragments_backward = nullptr;
    g_abi.composite_texture = reinterpret_cast<decltype(g_abi.composite_texture)>(dlsym(g_abi.handle, "dmr_composite_texture"));
    g_abi.composite_texture_backward =
        reinterpret_cast<decltype(g_abi.composite_texture_backward)>(dlsym(g_abi.handle, "dmr_composite_texture_backward"));
    if (!g_abi.composite_texture || !g_abi.composite_texture_backward) g_abi.composite_texture = nullptr, g_abi.composite_texture_backward = nullptr;
    g_abi.face_visibility = reinterpret_cast<decltype(g_abi.face_visibility)>(dlsym(g_abi.handle, "dmr_face_visibility"));
    g_abi.face_visibility_backward =
        reinterpret_cast<decltype(g_abi.face_visibility_backward)>(dlsym(g_abi.handle, "dmr_face_visibility_backward"));
    if (!g_abi.face_visibility || !g_abi.face_visibility_backward) g_abi.face_visibility = nullptr, g_abi.face_visibility_backward = nullptr;
    g_abi.interpolate_fragments = reinterpret_cast<decltype(g_abi.interpolate_fragments)>(dlsym(g_abi.handle, "dmr_interpolate_fragments"));
    g_abi.interpolate_fragments_backward =
        reinterpret_cast<decltype(g_abi.interpolate_fragments_backward)>(dlsym(g_abi.handle, "dmr_interpolate_fragments_backward"));
    g_abi.composite_values = reinterpret_cast<decltype(g_abi.composite_values)>(dlsym(g_abi.handle, "dmr_composite_values"));
    g_abi.composite_values_backward =
        reinterpret_cast<decltype(g_abi.composite_values_backward)>(dlsym(g_abi.handle, "dmr_composite_values_backward"));
    if (!g_abi.interpolate_fragments || !g_abi.interpolate_fragments_backward || !g_abi.composite_values || !g_abi.composite_values_backward)
        g_abi.interpolate_fragments = nullptr, g_abi.interpolate_fragments_backward = nullptr, g_abi.composite_values = nullptr,
        g_abi.composite_values_backward = nullptr;
    g_abi.pack_slots = reinterpret_cast<decltype(g_abi.pack_slots)>(dlsym(g_abi.handle, "dmr_pack_slots"));
    g_abi.interpolate_packed = reinterpret_cast<decltype(g_abi.interpolate_packed)>(dlsym(g_abi.handle, "dmr_interpolate_packed"));
    g_abi.interpolate_packed_backward =
        reinterpret_cast<decltype(g_abi.interpolate_packed_backward)>(dlsym(g_abi.handle, "dmr_interpolate_packed_backward"));
    g_abi.composite_values_packed = reinterpret_cast<decltype(g_abi.composite_values_packed)>(dlsym(g_abi.handle, "dmr_composite_values_packed"));
    g_abi.composite_values_packed_backward =
        reinterpret_cast<decltype(g_abi.composite_values_packed_backward)>(dlsym(g_abi.handle, "dmr_composite_values_packed_backward"));
    if (!g_abi.pack_slots || !g_abi.interpolate_packed || !g_abi.interpolate_packed_backward || !g_abi.composite_values_packed ||
        !g_abi.composite_values_packed_backward)
        g_abi.pack_slots = nullptr, g_abi.interpolate_packed = nullptr, g_abi.interpolate_packed_backward = nullptr,
        g_abi.composite_values_packed = nullptr, g_abi.composite_values_packed_backward = nullptr;
    g_abi.mlp_rows = reinterpret_cast<decltype(g_abi.mlp_rows)>(dlsym(g_abi.handle, "dmr_mlp_rows"));
    g_abi.mlp_rows_backward = reinterpret_cast<decltype(g_abi.mlp_rows_backward)>(dlsym(g_abi.handle, "dmr_mlp_rows_backward"));
    if (!g_abi.mlp_rows || !g_abi.mlp_rows_backward) g_abi.mlp_rows = nullptr, g_abi.mlp_rows_backward = nullptr;
    g_abi.hashgrid_layout = reinterpret_cast<decltype(g_abi.hashgrid_layout)>(dlsym(g_abi.handle, "dmr_hashgrid_layout"));
    g_abi.hashgrid_rows = reinterpret_cast<decltype(g_abi.hashgrid_rows)>(dlsym(g_abi.handle, "dmr_hashgrid_rows"));
    g_abi.hashgrid_rows_backward = reinterpret_cast<decltype(g_abi.hashgrid_rows_backward)>(dlsym(g_abi.handle, "dmr_hashgrid_rows_backward"));
    if (!g_abi.hashgrid_layout || !g_abi.hashgrid_rows || !g_abi.hashgrid_rows_backward)
        g_abi.hashgrid_layout = nullptr, g_abi.hashgrid_rows = nullptr, g_abi.hashgrid_rows_backward = nullptr;
    g_abi.packed_row_views = reinterpret_cast<decltype(g_abi.packed_row_views)>(dlsym(g_abi.handle, "dmr_packed_row_views"));
    g_abi.sh_rows = reinterpret_cast<decltype(g_abi.sh_rows)>(dlsym(g_abi.handle, "dmr_sh_rows"));
    g_abi.sh_rows_backward = reinterpret_cast<decltype(g_abi.sh_rows_backward)>(dlsym(g_abi.handle, "dmr_sh_rows_backward"));
    if (!g_abi.packed_row_views || !g_abi.sh_rows || !g_abi.sh_rows_backward)
        g_abi.packed_row_views = nullptr, g_abi.sh_rows = nullptr, g_abi.sh_rows_backward = nullptr;
    g_abi.envmap_rows = reinterpret_cast<decltype(g_abi.envmap_rows)>(dlsym(g_abi.handle, "dmr_envmap_rows"));
    g_abi.envmap_rows_backward = reinterpret_cast<decltype(g_abi.envmap_rows_backward)>(dlsym(g_abi.handle, "dmr_envmap_rows_backward"));
    if (!g_abi.envmap_rows || !g_abi.envmap_rows_backward) g_abi.envmap_rows = nullptr, g_abi.envmap_rows_backward = nullptr;
    g_abi.envmap_pyramid = reinterpret_cast<decltype(g_abi.envmap_pyramid)>(dlsym(g_abi.handle, "dmr_envmap_pyramid"));
    g_abi.envmap_pyramid_backward = reinterpret_cast<decltype(g_abi.envmap_pyramid_backward)>(dlsym(g_abi.handle, "dmr_envmap_pyramid_backward"));
    g_abi.envmap_lod_rows = reinterpret_cast<decltype(g_abi.envmap_lod_rows)>(dlsym(g_abi.handle, "dmr_envmap_lod_rows"));
    g_abi.envmap_lod_rows_backward = reinterpret_cast<decltype(g_abi.envmap_lod_rows_backward)>(dlsym(g_abi.handle, "dmr_envmap_lod_rows_backward"));
    if (!g_abi.envmap_pyramid || !g_abi.envmap_pyramid_backward || !g_abi.envmap_lod_rows || !g_abi.envmap_lod_rows_backward)
        g_abi.envmap_pyramid = nullptr, g_abi.envmap_pyramid_backward = nullptr, g_abi.envmap_lod_rows = nullptr, g_abi.envmap_lod_rows_backward = nullptr;
    g_abi.surface_packed = reinterpret_cast<decltype(g_abi.surface_packed)>(dlsym(g_abi.handle, "dmr_surface_packed"));
    g_abi.surface_packed_backward = reinterpret_cast<decltype(g_abi.surface_packed_backward)>(dlsym(g_abi.handle, "dmr_surface_packed_backward"));
    if (!g_abi.surface_packed || !g_abi.surface_packed_backward) g_abi.surface_packed = nullptr, g_abi.surface_packed_backward = nullptr;
    if (g_abi.abi_version() != DMR_ABI_VERSION)
        throw std::runtime_error("ABI mismatch: " + path + " is version " + std::to_string(g_abi.abi_version()) +
                                 ", the binding expects " + std::to_string(DMR_ABI_VERSION));
}

[[noreturn]] void raise_lib() { err(g_abi.last_error()); }

// ---- argument handling (render.cu:49-79,113-129,237-277) ------------------------------------------------------------
std::string dtype_name(const at::Tensor& t) { return std::string("torch.") + c10::toString(t.scalar_type()); }

at::Tensor f32(const at::Tensor& t, const char* name) {
    // render.cu:113-129: `.contiguous().data<float>()` throws for any other dtype
    if (t.scalar_type() != at::kFloat) err("expected scalar type Float but found " + dtype_name(t) + " (" + name + ")");
    return t.contiguous();
}
at::Tensor i32(const at::Tensor& t, const char* name) {
    if (t.scalar_type() != at::kInt) err("expected scalar type Int but found " + dtype_name(t) + " (" + name + ")");
    return t.contiguous();
}
// [B,4,4] matrix -> (tensor to keep alive, transposed-storage flag).  render.cu:117-120 makes the `.transpose(1, 2)`
// views of the wrapper contiguous with four copy kernels per call; the library reads that storage in place instead
// (dmr_scene.mats_transposed).
std::pair<at::Tensor, int> mat(const at::Tensor& t, const char* name) {
    if (t.scalar_type() != at::kFloat) err("expected scalar type Float but found " + dtype_name(t) + " (" + name + ")");
    if (t.is_contiguous()) return {t, 0};
    if (t.dim() == 3 && t.transpose(1, 2).is_contiguous()) return {t, 1};
    return {t.contiguous(), 0};
}

using In = const at::Tensor&;

// The tensors every render_* function starts with (and the tet renderer's three more, else null).
struct Inputs {
    In background, verts, faces, verts_color, faces_opacity, mv, proj, inv_mv, inv_proj, verts_depth, faces_intense;
    const at::Tensor *tets = nullptr, *face_tets = nullptr, *tet_faces = nullptr;
};

void check_common(const Inputs& in, bool tet) {
    const auto& [bg, verts, faces, verts_color, faces_opacity, mv, proj, inv_mv, inv_proj, verts_depth, faces_intense, tets, face_tets, tet_faces] = in;
    // messages: render.cu:49-79 (tri) and :237-267 (tet)
    if (verts.dim() != 2 || verts.size(1) != 3) err("verts must have dimensions (num_points, 3)");
    if (faces.dim() != 2 || faces.size(1) != 3) err("faces must have dimensions (num_faces, 3)");
    if (tet) {
        if (verts_color.dim() != 2 || verts_color.size(0) != verts.size(0) || verts_color.size(1) != 3)
            err("vert_color must have dimensions (num_verts, 3)");
        if (faces_opacity.dim() != 1 || faces_opacity.size(0) != faces.size(0)) err("face_opacity must have dimensions (num_faces)");
    } else {
        if (verts_color.dim() != 2 || verts_color.size(0) != verts.size(0)) err("vert color must have dimensions (num_points, N)");
        if (verts_color.size(1) != NUM_CHANNELS) err("vert color must have dimensions (num_points, 3)");  // Q15
        if (faces_opacity.dim() != 1 || faces_opacity.size(0) != faces.size(0)) err("face opacity must have dimensions (num_faces,)");
    }
    const std::string bdim = tet ? "batch_size" : "B";
    const std::pair<const at::Tensor*, const char*> mats[4] = {{&mv, "mv_mats"}, {&proj, "proj_mats"}, {&inv_mv, "inv_mv_mats"},
                                                               {&inv_proj, "inv_proj_mats"}};
    for (auto& m : mats)
        if (m.first->dim() != 3 || m.first->size(1) != 4 || m.first->size(2) != 4)
            err(std::string(m.second) + " must have dimensions (" + bdim + ", 4, 4)");
    if (verts_depth.dim() != 2 || verts_depth.size(1) != verts.size(0))
        err(tet ? "verts_depth must have dimensions (batch_size, num_verts)" : "verts_depth must have dimensions (B, num_points,)");
    if (faces_intense.dim() != 2 || faces_intense.size(1) != faces.size(0))
        err(tet ? "faces_intense must have dimensions (batch_size, num_faces)" : "faces_intense must have dimensions (B, num_faces,)");
    const int64_t B = mv.size(0);
    const std::pair<const at::Tensor*, const char*> batched[5] = {{&proj, "proj_mats"}, {&inv_mv, "inv_mv_mats"},
                                                                  {&inv_proj, "inv_proj_mats"}, {&verts_depth, "verts_depth"},
                                                                  {&faces_intense, "faces_intense"}};
    for (auto& m : batched)
        if (m.first->size(0) != B)  // the reference would read out of bounds here
            err(std::string(m.second) + " must have the batch size of mv_mats (" + std::to_string(B) + ")");
    if (!tet) return;
    // render.cu:269-277
    if (tets->dim() != 2 || tets->size(1) != 4) err("tets must have dimensions (num_tets, 4)");
    if (face_tets->dim() != 2 || face_tets->size(0) != faces.size(0) || face_tets->size(1) != 2) err("face_tets must have dimensions (num_faces, 2)");
    if (tet_faces->dim() != 2 || tet_faces->size(0) != tets->size(0) || tet_faces->size(1) != 4) err("tet_faces must have dimensions (num_tets, 4)");
}

c10::Device hip_device_of(const at::Tensor& verts) {
    if (!verts.is_cuda())
        err("dmesh_renderer_amd has no CPU path: tensors must be on a HIP device "
            "(the reference allocates on torch::kCUDA unconditionally, render.cu:91-96)");
    return verts.device();
}

at::TensorOptions f32_on(c10::Device dev) { return at::TensorOptions().dtype(at::kFloat).device(dev); }
void* stream_on(c10::Device dev) { return reinterpret_cast<void*>(c10::hip::getCurrentHIPStream(dev.index()).stream()); }  // PyTorch's current stream

// the caller-owned buffers of one call, by DMR_BUF_* id.  Up to DMR_BUF_WORK scratch, allocated on request: the C equivalent of
// the reference's four resizeFunctional lambdas (render.cu:18-24,91-100), plus the backward's transient workspace.  Beyond it
// the gradient outputs the library asks for (GradTable::from): tensors the backward has put here for the library to fill.
struct Scratch {
    c10::Device dev;
    std::array<at::Tensor, DMR_BUF_TET_FRAGMENT_BARY_GRADS + 1> buf;
    explicit Scratch(c10::Device d) : dev(d) {}
    at::Tensor get(int which) const {
        return buf[which].defined() ? buf[which] : at::empty({0}, at::TensorOptions().dtype(at::kByte).device(dev));
    }
};
void* alloc_cb(void* ctx, int which, size_t nbytes) {
    auto* s = reinterpret_cast<Scratch*>(ctx);
    if (which < 0 || which >= (int)s->buf.size()) return nullptr;
    if (which > DMR_BUF_WORK) {  // the caller's tensor (4-byte elements): an output the library fills (gradients, fragments) or an
                                 // input it reads (the fragment lists of fragment_grads=)
        const at::Tensor& t = s->buf[which];
        return t.defined() && (size_t)t.numel() * sizeof(float) >= nbytes ? t.data_ptr() : nullptr;
    }
    try {
        s->buf[which] = at::empty({(int64_t)std::max<size_t>(nbytes, 1)}, at::TensorOptions().dtype(at::kByte).device(s->dev));
        return s->buf[which].data_ptr();
    } catch (...) {  // reported by the library as an allocation failure
        return nullptr;
    }
}

// Owns the contiguous input tensors and the dmr_scene of one call.
struct Call {
    c10::Device dev;
    std::vector<at::Tensor> keep;
    dmr_scene sc{};
    Scratch scratch;

    template <class T>
    const T* ptr(const at::Tensor& t) { keep.push_back(t); return t.numel() ? reinterpret_cast<const T*>(t.data_ptr()) : nullptr; }

    Call(c10::Device dev_, const Inputs& in, int64_t H, int64_t W, int64_t seed, std::pair<int, int> rows) : dev(dev_), scratch(dev_) {
        const auto& [bg, verts, faces, verts_color, faces_opacity, mv, proj, inv_mv, inv_proj, verts_depth, faces_intense, tets, face_tets, tet_faces] = in;
        keep.reserve(16);
        auto m0 = mat(mv, "mv_mats"), m1 = mat(proj, "proj_mats"), m2 = mat(inv_mv, "inv_mv_mats"), m3 = mat(inv_proj, "inv_proj_mats");
        if (bg.numel() < NUM_CHANNELS) err("background must have 3 channels");
        sc.B = (int32_t)mv.size(0); sc.P = (int32_t)verts.size(0); sc.F = (int32_t)faces.size(0);
        sc.T = tets ? (int32_t)tets->size(0) : 0;
        sc.W = (int32_t)W; sc.H = (int32_t)H;
        sc.background = ptr<float>(f32(bg, "background"));
        sc.verts = ptr<float>(f32(verts, "verts"));
        sc.faces = ptr<int32_t>(i32(faces, "faces"));
        sc.verts_color = ptr<float>(f32(verts_color, "verts_color"));
        sc.faces_opacity = ptr<float>(f32(faces_opacity, "faces_opacity"));
        sc.mv_mats = ptr<float>(m0.first); sc.proj_mats = ptr<float>(m1.first);
        sc.inv_mv_mats = ptr<float>(m2.first); sc.inv_proj_mats = ptr<float>(m3.first);
        sc.verts_depth = ptr<float>(f32(verts_depth, "verts_depth"));
        sc.faces_intense = ptr<float>(f32(faces_intense, "faces_intense"));
        if (tets) {
            sc.tets = ptr<int32_t>(i32(*tets, "tets"));
            sc.face_tets = ptr<int32_t>(i32(*face_tets, "face_tets"));
            sc.tet_faces = ptr<int32_t>(i32(*tet_faces, "tet_faces"));
        }
        sc.ray_random_seed = (int32_t)seed;
        sc.row_begin = rows.first; sc.row_end = rows.second;
        sc.mats_transposed = m0.second | (m1.second << 1) | (m2.second << 2) | (m3.second << 3);
        sc.flags = g_async.load(std::memory_order_relaxed) ? DMR_FLAG_ASYNC : 0;
        for (const at::Tensor& t : keep)
            if (t.device() != dev) err("all tensors must be on " + dev.str() + " (one is on " + t.device().str() + ")");
    }

    void* stream() const { return stream_on(dev); }
};

template <class T> T* mptr(const at::Tensor& t) { return t.numel() ? reinterpret_cast<T*>(t.data_ptr()) : nullptr; }

// ---- the four functions of ext.cpp:6-11 -----------------------------------------------------------------------------
// What the two forwards share: the call, color [B,3,H,W] and depth [B,1,H,W] -- with alpha=True (DMR_FLAG_ALPHA) [B,2,H,W],
// depth | alpha, channel 1 the accumulated opacity alpha = 1 - T_final -- and the return of the four scratch buffers.
struct Forward {
    c10::Device dev;
    c10::DeviceGuard guard;
    Call call;
    // the kernels write every pixel of the rendered rows (tet: the background where the march fails); zero-fill (render.cu:88-89,
    // :287-290) is only needed when nothing is launched (P == 0 / F == 0, render.cu:105) or when a band leaves rows untouched
    bool written;
    at::Tensor color, depth;

    Forward(const Inputs& in, int64_t H, int64_t W, int64_t seed, std::pair<int, int> rows, bool fill_outside, bool alpha)
        : dev(hip_device_of(in.verts)), guard(dev), call(dev, in, H, W, seed, rows),
          written(((rows.first == 0 && rows.second == 0) || !fill_outside) && call.sc.P > 0 && call.sc.F > 0),
          color(image({call.sc.B, NUM_CHANNELS, H, W})), depth(image({call.sc.B, alpha ? 2 : 1, H, W})) {
        if (alpha) call.sc.flags |= DMR_FLAG_ALPHA;
    }
    at::Tensor image(at::IntArrayRef shape) const { return written ? at::empty(shape, f32_on(dev)) : at::zeros(shape, f32_on(dev)); }
    template <class... Out>  // -> (out..., pointBuffer, faceBuffer, binningBuffer, imgBuffer)
    auto result(Out... out) const {
        return std::make_tuple(out..., call.scratch.get(DMR_BUF_POINT), call.scratch.get(DMR_BUF_FACE), call.scratch.get(DMR_BUF_BINNING),
                               call.scratch.get(DMR_BUF_IMAGE));
    }
};

// A renderer's fragment ids in the C ABI: the forward's flag and its one output buffer, the backward's flag and its two inputs.
struct FragmentIds { int flag, buf, grads_flag, faces_buf, grads_buf; };
constexpr FragmentIds TRI_FRAGMENTS{DMR_FLAG_TRI_FRAGMENTS, DMR_BUF_TRI_FRAGMENTS, DMR_FLAG_TRI_FRAGMENT_GRADS, DMR_BUF_TRI_FRAGMENT_FACES,
                                    DMR_BUF_TRI_FRAGMENT_BARY_GRADS};
constexpr FragmentIds TET_FRAGMENTS{DMR_FLAG_TET_FRAGMENTS, DMR_BUF_TET_FRAGMENTS, DMR_FLAG_TET_FRAGMENT_GRADS, DMR_BUF_TET_FRAGMENT_FACES,
                                    DMR_BUF_TET_FRAGMENT_BARY_GRADS};

// The fragment lists of render_tris / render_tets(fragments=K): ONE buffer [face i32 B,K,H,W | bary f32 B,K,2,H,W | count i32
// B,H,W] -- what the library requests as ids.buf when ids.flag is set -- and its three pieces as views.  Pre-initialised (face
// -1, the rest 0) for the images' reason: a row band, or P == 0 / F == 0, where nothing writes them (Forward::written).
// K == 0: no request, three undefined tensors.
struct Fragments {
    at::Tensor face, bary, count;
    Fragments(Forward& f, const FragmentIds& ids, int64_t K, int64_t H, int64_t W) {
        if (K == 0) return;
        const int64_t B = f.call.sc.B, n = B * H * W;
        const at::Tensor buf = at::empty({n * (3 * K + 1)}, at::TensorOptions().dtype(at::kInt).device(f.dev));
        face = buf.narrow(0, 0, K * n).view({B, K, H, W});
        bary = buf.narrow(0, K * n, 2 * K * n).view(at::kFloat).view({B, K, 2, H, W});
        count = buf.narrow(0, 3 * K * n, n).view({B, H, W});
        if (!f.written) { face.fill_(-1); buf.narrow(0, K * n, (2 * K + 1) * n).zero_(); }
        f.call.scratch.buf[ids.buf] = buf;
        f.call.sc.flags |= ids.flag | ((int)K << 8);
    }
    auto tuple() const { return std::make_tuple(face, bary, count); }
};

void check_fragments(int64_t fragments) {
    if (fragments < 0 || fragments > 32) err("fragments must be in 0..32 (fragment slots per pixel; 0: no fragment output), got " + std::to_string(fragments));
}

// -> (num_rendered:int, color, depth, pointBuffer, faceBuffer, binningBuffer, imgBuffer, face, bary, count): the last three
// undefined tensors unless fragments=K > 0.  (Bound below through bind_forward.)
using TriFwdOut = std::tuple<int64_t, at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor>;
TriFwdOut render_tris(In background, In verts, In faces, In verts_color, In faces_opacity, In mv_mats, In proj_mats, In inv_mv_mats,
                      In inv_proj_mats, In verts_depth, In faces_intense, int64_t image_height, int64_t image_width, std::pair<int, int> rows,
                      bool fill_outside, bool alpha, int64_t fragments) {
    const Inputs in{background, verts, faces, verts_color, faces_opacity, mv_mats, proj_mats, inv_mv_mats, inv_proj_mats, verts_depth, faces_intense};
    check_common(in, false);
    check_fragments(fragments);
    Forward f(in, image_height, image_width, 0, rows, fill_outside, alpha);
    const Fragments frag(f, TRI_FRAGMENTS, fragments, image_height, image_width);
    int rendered = 0;
    // (the bindings release the GIL around this whole function: the default call waits for the size read-back)
    if (g_abi.tri_forward(&f.call.sc, mptr<float>(f.color), mptr<float>(f.depth), &alloc_cb, &f.call.scratch, f.call.stream(), &rendered)) raise_lib();
    return std::tuple_cat(f.result((int64_t)rendered, f.color, f.depth), frag.tuple());
}

// -> (color, depth, active f32 [B,H,W], pointBuffer, faceBuffer, binningBuffer, imgBuffer, face, bary, count): the last three
// undefined tensors unless fragments=K > 0 (bound below like render_tris)
using TetFwdOut = std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor>;
TetFwdOut render_tets(In background, In verts, In faces, In verts_color, In faces_opacity, In mv_mats, In proj_mats, In inv_mv_mats,
                      In inv_proj_mats, In verts_depth, In faces_intense, In tets, In face_tets, In tet_faces, int64_t image_height,
                      int64_t image_width, int64_t ray_random_seed, std::pair<int, int> rows, bool alpha, int64_t fragments) {
    const Inputs in{background, verts, faces, verts_color, faces_opacity, mv_mats, proj_mats, inv_mv_mats, inv_proj_mats, verts_depth, faces_intense,
                    &tets, &face_tets, &tet_faces};
    check_common(in, true);
    check_fragments(fragments);
    Forward f(in, image_height, image_width, ray_random_seed, rows, true, alpha);
    const at::Tensor active = f.image({f.call.sc.B, image_height, image_width});
    const Fragments frag(f, TET_FRAGMENTS, fragments, image_height, image_width);
    int rendered = 0;
    if (g_abi.tet_forward(&f.call.sc, mptr<float>(f.color), mptr<float>(f.depth), mptr<float>(active), &alloc_cb, &f.call.scratch, f.call.stream(),
                          &rendered))
        raise_lib();
    return std::tuple_cat(f.result(f.color, f.depth, active), frag.tuple());
}

// ---- the gradient set of a backward, stated once ------------------------------------------------------------------------
// Level 0: the reference's gradients; 1: exact_grads (tri) / full_grads (tet); 2: camera_grads, which implies level 1.
// `shape`: the pieces of the flat layout, in its order -- what flat_out holds back to back (the payload of the one all-reduce
// in sharding.py, which states the same table: _TRI_GRADS / _TET_GRADS) and what is allocated otherwise.  `from`: where the
// library gets a piece's pointer: ARG, the next gradient argument of the C call, or the DMR_BUF_* id of the output it requests
// through alloc (alloc_cb serves it from Scratch::buf; consecutive pieces of one id are one buffer).  `tuple`: the pieces in
// the order of the returned tuple; a [B, n, 4, 4] piece -- n matrix gradients per view in the library's contract layout
// m[4*col+row] -- stands for its n [B,4,4] slices: element [b,i,j] is the gradient of the matrix tensor's [b,i,j] as the call
// received it (the contract layout read as a row-major [4,4] is the transpose of the matrix it means, which is how such a
// tensor holds it).  `flags`: the level's DMR_FLAG_* bits.
constexpr int ARG = -1;
using Shape = c10::SmallVector<int64_t, 4>;
struct GradTable {
    c10::SmallVector<Shape, 6> shape;
    c10::SmallVector<int, 6> from, tuple;
    int flags;
    void add(Shape s, int buf) { tuple.push_back((int)shape.size()); shape.push_back(std::move(s)); from.push_back(buf); }
};

// -> (dL_dverts, dL_dvcolor, dL_dfopacity, dL_dvdepth, dL_dfintense), camera: then (dL_dinv_mv_mats, dL_dinv_proj_mats).
// Level 0 is exactly the reference's function (render.cu:134-208).
GradTable tri_grads(int level, int64_t P, int64_t F, int64_t B) {
    static const int flags[3] = {0, DMR_FLAG_TRI_EXACT_GRADS, DMR_FLAG_TRI_EXACT_GRADS | DMR_FLAG_TRI_CAMERA_GRADS};
    GradTable t{{{P, 3}, {P, NUM_CHANNELS}, {F}, {B, P}, {B, F}}, {ARG, ARG, ARG, ARG, ARG}, {0, 1, 2, 3, 4}, flags[level]};
    if (level == 2) t.add({B, 2, 4, 4}, DMR_BUF_TRI_CAMERA_GRADS);
    return t;
}

// -> (dL_dverts_color, dL_dfaces_opacity); full: (dL_dverts, dL_dverts_color, dL_dfaces_opacity, dL_dfaces_intense); camera: then
// (dL_dinv_mv_mats, dL_dinv_proj_mats, dL_dmv_mats, dL_dproj_mats).  Level 0 is exactly the reference's function (render.cu:338-412).
GradTable tet_grads(int level, int64_t P, int64_t F, int64_t B) {
    static const int flags[3] = {0, DMR_FLAG_TET_FULL_GRADS, DMR_FLAG_TET_FULL_GRADS | DMR_FLAG_TET_CAMERA_GRADS};
    GradTable t{{{P, 3}, {F}}, {ARG, ARG}, {0, 1}, flags[level]};
    if (level >= 1) {
        t.add({P, 3}, DMR_BUF_TET_GRADS);  // [dL_dverts 3P | dL_dfaces_intense BF]: one buffer
        t.add({B, F}, DMR_BUF_TET_GRADS);
        t.tuple = {2, 0, 1, 3};
    }
    if (level == 2) t.add({B, 4, 4, 4}, DMR_BUF_TET_CAMERA_GRADS);
    return t;
}

// The pieces of `t` as tensors: each run (a piece, or the pieces of one buffer) allocated, or carved in order out of flat_out,
// the caller's buffer, which must hold exactly all of them.  A run the library requests is left where alloc_cb finds it.
std::vector<at::Tensor> grad_outputs(Call& call, const std::optional<at::Tensor>& flat_out, const GradTable& t) {
    const size_t n = t.shape.size();
    c10::SmallVector<int64_t, 6> numel;
    int64_t total = 0;
    for (const Shape& s : t.shape) total += numel.emplace_back(c10::multiply_integers(s));
    at::Tensor flat;
    if (flat_out.has_value()) {
        const at::Tensor& fo = *flat_out;
        if (fo.scalar_type() != at::kFloat || fo.device() != call.dev || !fo.is_contiguous() || fo.numel() != total)
            err("flat_out must be a contiguous float32 tensor of " + std::to_string(total) + " elements on " + call.dev.str());
        flat = fo.view({-1});
    }
    std::vector<at::Tensor> g(n);
    int64_t o = 0;
    for (size_t i = 0, j; i < n; i = j) {
        int64_t len = numel[i];
        for (j = i + 1; j < n && t.from[i] != ARG && t.from[j] == t.from[i]; j++) len += numel[j];
        const bool one = j == i + 1;
        const at::Tensor run = flat.defined() ? flat.narrow(0, o, len) : at::empty(one ? at::IntArrayRef(t.shape[i]) : at::IntArrayRef(len), f32_on(call.dev));
        if (t.from[i] != ARG) call.scratch.buf[t.from[i]] = run;
        for (int64_t k = 0; i < j; k += numel[i++]) {
            const at::Tensor piece = one ? run : run.narrow(0, k, numel[i]);
            g[i] = piece.sizes() == at::IntArrayRef(t.shape[i]) ? piece : piece.view(t.shape[i]);
        }
        o += len;
    }
    return g;
}

// The body of the two backwards: `launch(call, dL_dcolor, dL_ddepth, the four scratch buffers, the ARG pieces)` is the C call.
template <class Launch>
py::tuple backward(const Inputs& in, In grad_color, In grad_depth, const char* color_name, const char* depth_name, In pointBuffer, In faceBuffer,
                   In binningBuffer, In imageBuffer, std::pair<int, int> rows, const std::optional<at::Tensor>& flat_out,
                   GradTable (*table)(int, int64_t, int64_t, int64_t), int level, bool alpha, Launch launch) {
    std::optional<py::gil_scoped_release> nogil(std::in_place);  // (the default call waits for the size read-back)
    const c10::Device dev = hip_device_of(in.verts);
    c10::DeviceGuard guard(dev);
    if (grad_color.dim() != 4) err(std::string(color_name) + " must have dimensions (B, 3, H, W)");
    const int64_t H = grad_color.size(2), W = grad_color.size(3);  // render.cu:163-164, :371-372
    Call call(dev, in, H, W, 0, rows);
    const at::Tensor gc = f32(grad_color, color_name);  // may arrive non-contiguous / expanded (render.cu:197-198)
    const at::Tensor gd = f32(grad_depth, depth_name);
    if (alpha) {  // [B,2,H,W], depth | alpha
        if (gd.dim() != 4 || gd.size(0) != call.sc.B || gd.size(1) != 2 || gd.size(2) != H || gd.size(3) != W)
            err(std::string(depth_name) + " must have dimensions (B, 2, H, W) with alpha=True (channel 0 the depth's gradient, channel 1 "
                "alpha's): (" + std::to_string(call.sc.B) + ", 2, " + std::to_string(H) + ", " + std::to_string(W) + ") here");
        call.sc.flags |= DMR_FLAG_ALPHA;
    }
    const GradTable t = table(level, call.sc.P, call.sc.F, call.sc.B);
    call.sc.flags |= t.flags;
    const std::vector<at::Tensor> g = grad_outputs(call, flat_out, t);
    float* args[5];
    for (size_t i = 0, a = 0; i < g.size(); i++)
        if (t.from[i] == ARG) args[a++] = mptr<float>(g[i]);
    const at::Tensor buf[4] = {pointBuffer.contiguous(), faceBuffer.contiguous(), binningBuffer.contiguous(), imageBuffer.contiguous()};
    const void* bufs[4] = {mptr<const void>(buf[0]), mptr<const void>(buf[1]), mptr<const void>(buf[2]), mptr<const void>(buf[3])};
    if (launch(call, mptr<const float>(gc), mptr<const float>(gd), bufs, args)) raise_lib();
    std::vector<at::Tensor> out;
    for (int i : t.tuple) {
        if (t.shape[i].size() != 4) out.push_back(g[i]);
        else for (int64_t k = 0; k < t.shape[i][1]; k++) out.push_back(g[i].select(1, k));
    }
    nogil.reset();
    return py::tuple(py::cast(out));
}

// fragment_grads=(pix_to_face, grad_bary) of render_tris_backward / render_tets_backward: checked, then handed to the library as
// they are (the two input buffers it requests, ids.faces_buf and ids.grads_buf; alloc_cb serves them from Scratch::buf) with
// ids.grads_flag and K.
using FragmentGrads = std::optional<std::pair<at::Tensor, at::Tensor>>;
void attach_fragment_grads(Call& c, const FragmentIds& ids, const FragmentGrads& fg, int64_t H, int64_t W) {
    if (!fg.has_value()) return;
    const at::Tensor& face = fg->first;
    const at::Tensor& grad = fg->second;
    if (!face.defined() || !grad.defined()) err("fragment_grads must be (pix_to_face, grad_bary), two tensors");
    if (face.device() != c.dev || grad.device() != c.dev)
        err("fragment_grads: pix_to_face and grad_bary must be on " + c.dev.str() + " (they are on " + face.device().str() + ", " +
            grad.device().str() + ")");
    if (face.scalar_type() != at::kInt) err("fragment_grads: pix_to_face must be int32, found " + dtype_name(face));
    if (grad.scalar_type() != at::kFloat) err("fragment_grads: grad_bary must be float32, found " + dtype_name(grad));
    const int64_t B = c.sc.B, K = face.dim() == 4 ? face.size(1) : 0;
    if (face.dim() != 4 || face.size(0) != B || face.size(2) != H || face.size(3) != W || K < 1 || K > 32)
        err("fragment_grads: pix_to_face must have dimensions (B, K, H, W) = (" + std::to_string(B) + ", 1..32, " + std::to_string(H) + ", " +
            std::to_string(W) + ")");
    if (grad.dim() != 5 || grad.size(0) != B || grad.size(1) != K || grad.size(2) != 2 || grad.size(3) != H || grad.size(4) != W)
        err("fragment_grads: grad_bary must have dimensions (B, K, 2, H, W) = (" + std::to_string(B) + ", " + std::to_string(K) + ", 2, " +
            std::to_string(H) + ", " + std::to_string(W) + ")");
    if (!face.is_contiguous() || !grad.is_contiguous()) err("fragment_grads: pix_to_face and grad_bary must be contiguous");
    c.scratch.buf[ids.faces_buf] = face;
    c.scratch.buf[ids.grads_buf] = grad;
    c.sc.flags |= ids.grads_flag | ((int)K << 8);
}

// tri_grads' tuple; the keywords select its level
py::tuple render_tris_backward(In background, In verts, In faces, In verts_color, In faces_opacity, In mv_mats, In proj_mats, In inv_mv_mats,
                               In inv_proj_mats, In verts_depth, In faces_intense, In dL_dout_color, In dL_dout_depth, int64_t R, In pointBuffer,
                               In faceBuffer, In binningBuffer, In imageBuffer, std::pair<int, int> rows, const std::optional<at::Tensor>& flat_out,
                               bool exact_grads, bool camera_grads, bool alpha, const FragmentGrads& fragment_grads) {
    return backward({background, verts, faces, verts_color, faces_opacity, mv_mats, proj_mats, inv_mv_mats, inv_proj_mats, verts_depth, faces_intense},
                    dL_dout_color, dL_dout_depth, "dL_dout_color", "dL_dout_depth", pointBuffer, faceBuffer, binningBuffer, imageBuffer, rows, flat_out,
                    &tri_grads, camera_grads ? 2 : exact_grads, alpha,
                    [R, &fragment_grads](Call& c, const float* gc, const float* gd, const void* const* b, float* const* g) {
                        attach_fragment_grads(c, TRI_FRAGMENTS, fragment_grads, c.sc.H, c.sc.W);
                        return g_abi.tri_backward(&c.sc, gc, gd, (int)R, b[0], b[1], b[2], b[3], g[0], g[1], g[2], g[3], g[4], &alloc_cb, &c.scratch,
                                                  c.stream());
                    });
}

// tet_grads' tuple; the keywords select its level (fragment_grads: at least 1 -- dL_dverts exists from there on)
py::tuple render_tets_backward(In background, In verts, In faces, In verts_color, In faces_opacity, In mv_mats, In proj_mats, In inv_mv_mats,
                               In inv_proj_mats, In verts_depth, In faces_intense, In tets, In face_tets, In tet_faces, In grad_color, In grad_depth,
                               In pointBuffer, In faceBuffer, In binningBuffer, In imageBuffer, std::pair<int, int> rows,
                               const std::optional<at::Tensor>& flat_out, bool full_grads, bool camera_grads, bool alpha,
                               const FragmentGrads& fragment_grads) {
    return backward({background, verts, faces, verts_color, faces_opacity, mv_mats, proj_mats, inv_mv_mats, inv_proj_mats, verts_depth, faces_intense,
                     &tets, &face_tets, &tet_faces},
                    grad_color, grad_depth, "grad_color", "grad_depth", pointBuffer, faceBuffer, binningBuffer, imageBuffer, rows, flat_out, &tet_grads,
                    camera_grads ? 2 : (full_grads || fragment_grads.has_value()), alpha,
                    [&fragment_grads](Call& c, const float* gc, const float* gd, const void* const* b, float* const* g) {
                        attach_fragment_grads(c, TET_FRAGMENTS, fragment_grads, c.sc.H, c.sc.W);
                        return g_abi.tet_backward(&c.sc, gc, gd, b[0], b[1], b[2], b[3], g[0], g[1], &alloc_cb, &c.scratch, c.stream());
                    });
}

// ---- extensions -----------------------------------------------------------------------------------------------------
// th.inverse of [B,4,4] float32 HIP tensors with one small library kernel each (dmr_invert_mats: adjugate in double
// precision).  The reference wrapper calls th.inverse twice per forward (dmesh_renderer/__init__.py:62-63: two batched
// LU factorisations, ~0.12 ms of small kernels on the GPU).  Returns contiguous tensors.
py::tuple invert_mats(const py::args& mats) {
    if (mats.size() == 0) return py::tuple();
    std::vector<at::Tensor> in;
    for (const auto& h : mats) in.push_back(h.cast<at::Tensor>());
    const c10::Device dev = hip_device_of(in[0]);
    c10::DeviceGuard guard(dev);
    void* st = stream_on(dev);
    py::tuple res(in.size());
    for (size_t i = 0; i < in.size(); i++) {
        const at::Tensor& m = in[i];
        if (m.dim() != 3 || m.size(1) != 4 || m.size(2) != 4) err("matrices must have dimensions (B, 4, 4)");
        if (m.device() != dev) err("all matrices must be on " + dev.str());
        auto t = mat(m, "matrix");
        at::Tensor out = at::empty({t.first.size(0), 4, 4}, f32_on(dev));
        if (t.first.size(0) && g_abi.invert_mats(mptr<const float>(t.first), (int)t.first.size(0), t.second, mptr<float>(out), st)) raise_lib();
        res[i] = out;
    }
    return res;
}

// Parity/debug helper: copy one forward intermediate out of the scratch buffers (dmr_export).  `call_args` are the 11
// (tri) / 14 (tet) leading tensors of render_*.
at::Tensor export_item(const std::string& name, const py::sequence& call_args, bool is_tet, int64_t num_rendered,
                       const py::sequence& buffers, int64_t H, int64_t W, const py::object& dtype) {
    std::vector<at::Tensor> a;
    for (const auto& h : call_args) a.push_back(h.cast<at::Tensor>());
    if (a.size() < (is_tet ? 14u : 11u)) err("export: call_args must hold the leading tensors of render_*");
    const c10::Device dev = hip_device_of(a[1]);
    c10::DeviceGuard guard(dev);
    Call call(dev, {a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9], a[10], is_tet ? &a[11] : nullptr, is_tet ? &a[12] : nullptr,
                    is_tet ? &a[13] : nullptr}, H, W, 0, {0, 0});
    std::vector<at::Tensor> b;
    for (const auto& h : buffers) b.push_back(h.cast<at::Tensor>().contiguous());
    if (b.size() != 4) err("export: buffers must be the four scratch tensors");
    void* st = call.stream();
    const int64_t n = g_abi.export_item(&call.sc, is_tet ? 1 : 0, (int)num_rendered, name.c_str(), mptr<const void>(b[0]), mptr<const void>(b[1]),
                                        mptr<const void>(b[2]), mptr<const void>(b[3]), nullptr, 0, st);
    if (n < 0) raise_lib();
    at::Tensor out = at::empty({std::max<int64_t>(n, 1)}, at::TensorOptions().dtype(at::kByte).device(dev));
    g_abi.export_item(&call.sc, is_tet ? 1 : 0, (int)num_rendered, name.c_str(), mptr<const void>(b[0]), mptr<const void>(b[1]),
                      mptr<const void>(b[2]), mptr<const void>(b[3]), out.data_ptr(), n, st);
    return out.narrow(0, 0, n).view(torch::python::detail::py_object_to_dtype(dtype));
}

// ---- shading over fragment lists: composite_fragments* (dmesh_renderer_amd_shade.h), composite_texture* (.._texture.h),
// face_visibility* (.._visibility.h), interpolate_fragments* / composite_values* (.._deferred.h) and pack_slots /
// interpolate_packed* / composite_values_packed* (.._packed.h); fragments.py's *_fused functions ----------------------------------
// Every shading call starts from pix_to_face [B,K,H,W] on a HIP device: Lists.  A unit's argument block extends it with the
// unit's own tensors, checked and made contiguous by a builder that calls the named checks below in the unit's order, which is
// fragments.py's: the first check that fails decides the message (tests/golden/shading_refusals.json, "binding").
struct Lists {
    at::Tensor face;
    int64_t B = 0, K = 0, H = 0, W = 0;
    c10::Device dev{c10::kCPU};
    const char* call = "";  // what the unit's own messages start with: "composite_fragments", ...
    void* stream() const { return stream_on(dev); }
};
// ... and what the calls that blend add: the opacities [F] and the optional per-face scale [B,F] (undefined = none)
struct Blend {
    at::Tensor opacity, scale;
    int64_t F = 0;
    const float* scale_ptr() const { return scale.defined() ? mptr<const float>(scale) : nullptr; }
};

template <class Fn>
void built(Fn fn, const char* symbol) {
    if (!fn) err(g_abi.path + " does not export " + symbol + ": rebuild it (python -m dmesh_renderer_amd.build)");
}
// the device and B, K, H, W (face itself is kept once it is checked: the builder's last step)
void lists_begin(Lists& a, const char* call, In face) {
    a.call = call;
    a.dev = hip_device_of(face);
    if (face.dim() != 4) err("pix_to_face must have dimensions (B, K, H, W)");
    a.B = face.size(0); a.K = face.size(1); a.H = face.size(2); a.W = face.size(3);
}
void check_bary(const Lists& a, In bary) {
    if (bary.dim() != 5 || bary.size(0) != a.B || bary.size(1) != a.K || bary.size(2) != 2 || bary.size(3) != a.H || bary.size(4) != a.W)
        err("bary must have dimensions (B, K, 2, H, W) of pix_to_face's B, K, H, W");
}
// an [F,3] table of corners (faces / uv_faces) -> F
int64_t check_corners(In corners, const char* name) {
    if (corners.dim() != 2 || corners.size(1) != 3) err(std::string(name) + " must have dimensions (num_faces, 3)");
    return corners.size(0);
}
// faces_opacity [F] -> F; F < 0: any length
int64_t check_opacity(In faces_opacity, int64_t F = -1) {
    if (faces_opacity.dim() != 1 || (F >= 0 && faces_opacity.size(0) != F)) err("faces_opacity must have dimensions (num_faces,)");
    return faces_opacity.size(0);
}
// vert_attrs [P,C] -> P, C
void check_attrs(In vert_attrs, int64_t& P, int64_t& C) {
    if (vert_attrs.dim() != 2) err("vert_attrs must have dimensions (num_points, C)");
    P = vert_attrs.size(0); C = vert_attrs.size(1);
}
void check_scale(const Lists& a, int64_t F, const std::optional<at::Tensor>& face_scale) {
    if (face_scale && (face_scale->dim() != 2 || face_scale->size(0) != a.B || face_scale->size(1) != F))
        err("face_scale must have dimensions (B, num_faces)");
}
void check_k(const Lists& a) { if (a.K < 1 || a.K > 32) err(std::string(a.call) + ": K must be in 1..32, got " + std::to_string(a.K)); }
void check_c(const Lists& a, int64_t C, int64_t max_c) {
    if (C < 1 || C > max_c) err(std::string(a.call) + ": C must be in 1.." + std::to_string(max_c) + ", got " + std::to_string(C));
}
void check_not_empty(const Lists& a) { if (a.B < 1 || a.H < 1 || a.W < 1) err(std::string(a.call) + ": empty fragment lists"); }
void same_device(const Lists& a, In t, const char* name) {
    if (t.device() != a.dev) err(std::string(name) + " must be on the device of pix_to_face");
}
void same_device(const Lists& a, const std::optional<at::Tensor>& t, const char* name) { if (t) same_device(a, *t, name); }

// composite_fragments and composite_texture have the same lists -- barycentrics, the unit's [F,3] corner table, opacities,
// scale -- and tensors of their own between.  Such a unit calls list_dims, its own shape checks, check_k, its own size checks,
// check_not_empty, list_finish.
struct ListArgs : Lists, Blend {
    at::Tensor bary, corners;
    const char* corner_name = "";  // what the unit calls `corners`
};
struct OwnTensor { In in; const char* name; at::Tensor& out; };  // one of a unit's own f32 tensors, and where its contiguous form goes

void list_dims(ListArgs& a, const char* call, const char* corner_name, In face, In bary, In corners, In faces_opacity) {
    a.corner_name = corner_name;
    lists_begin(a, call, face);
    check_bary(a, bary);
    a.F = check_corners(corners, corner_name);
    check_opacity(faces_opacity, a.F);
    a.face = face; a.bary = bary; a.corners = corners; a.opacity = faces_opacity;
}
// face_scale's dimensions, one device for every tensor, then dtypes: the tensors of `a` and the unit's `own` made contiguous
void list_finish(ListArgs& a, const std::optional<at::Tensor>& face_scale, std::initializer_list<OwnTensor> own) {
    check_scale(a, a.F, face_scale);
    same_device(a, a.bary, "bary"); same_device(a, a.corners, a.corner_name); same_device(a, a.opacity, "faces_opacity");
    for (const OwnTensor& o : own) same_device(a, o.in, o.name);
    same_device(a, face_scale, "face_scale");
    a.face = i32(a.face, "pix_to_face"); a.bary = f32(a.bary, "bary"); a.corners = i32(a.corners, a.corner_name);
    a.opacity = f32(a.opacity, "faces_opacity");
    for (const OwnTensor& o : own) o.out = f32(o.in, o.name);
    if (face_scale) a.scale = f32(*face_scale, "face_scale");
}

// The two outputs of a compositing forward, image [B,C,H,W] and T [B,1,H,W] ...
std::tuple<at::Tensor, at::Tensor> image_and_T(const Lists& a, int64_t C) {
    return {at::empty({a.B, C, a.H, a.W}, f32_on(a.dev)), at::empty({a.B, 1, a.H, a.W}, f32_on(a.dev))};
}
// ... and the two upstreams of its backward, grad_image [B,C,H,W] / grad_T [B,1,H,W], checked and contiguous; undefined: None = zero.
std::pair<at::Tensor, at::Tensor> upstreams(const Lists& a, int64_t C, const std::optional<at::Tensor>& grad_image,
                                            const std::optional<at::Tensor>& grad_T) {
    at::Tensor gi, gt;
    if (grad_image) {
        if (grad_image->dim() != 4 || grad_image->size(0) != a.B || grad_image->size(1) != C || grad_image->size(2) != a.H ||
            grad_image->size(3) != a.W || grad_image->device() != a.dev)
            err("grad_image must have dimensions (B, C, H, W) on the device of pix_to_face");
        gi = f32(*grad_image, "grad_image");
    }
    if (grad_T) {
        if (grad_T->numel() != (int64_t)a.B * a.H * a.W || grad_T->device() != a.dev) err("grad_T must have dimensions (B, 1, H, W) on the device of pix_to_face");
        gt = f32(*grad_T, "grad_T");
    }
    return {gi, gt};
}

// an optional tensor as the C calls take it (null = none / not wanted) and as Python gets it back; a gradient output if asked for
const float* in_ptr(const at::Tensor& t) { return t.defined() ? mptr<const float>(t) : nullptr; }
float* out_ptr(at::Tensor& t) { return t.defined() ? mptr<float>(t) : nullptr; }
py::object or_none(const at::Tensor& t) { return t.defined() ? py::cast(t) : py::none(); }
at::Tensor grad_if(bool need, at::IntArrayRef shape, c10::Device dev) { return need ? at::empty(shape, f32_on(dev)) : at::Tensor(); }

// -- composite_fragments: per-vertex attributes
struct ShadeArgs : ListArgs { at::Tensor attrs; int64_t P = 0, C = 0; };

ShadeArgs shade_args(In face, In bary, In faces, In faces_opacity, In vert_attrs, const std::optional<at::Tensor>& face_scale) {
    built(g_abi.composite_fragments, "dmr_composite_fragments");
    ShadeArgs a;
    list_dims(a, "composite_fragments", "faces", face, bary, faces, faces_opacity);
    check_attrs(vert_attrs, a.P, a.C);
    check_k(a);
    check_c(a, a.C, 256);
    check_not_empty(a);
    list_finish(a, face_scale, {{vert_attrs, "vert_attrs", a.attrs}});
    return a;
}

// -> (image [B,C,H,W], T [B,1,H,W])
std::tuple<at::Tensor, at::Tensor> composite_fragments(In face, In bary, In faces, In faces_opacity, In vert_attrs,
                                                       const std::optional<at::Tensor>& face_scale) {
    const ShadeArgs a = shade_args(face, bary, faces, faces_opacity, vert_attrs, face_scale);
    c10::DeviceGuard guard(a.dev);
    auto [image, T] = image_and_T(a, a.C);
    if (g_abi.composite_fragments(a.B, a.K, a.H, a.W, a.P, a.F, a.C, mptr<const int32_t>(a.face), mptr<const float>(a.bary),
                                  mptr<const int32_t>(a.corners), mptr<const float>(a.opacity), mptr<const float>(a.attrs), a.scale_ptr(),
                                  mptr<float>(image), mptr<float>(T), a.stream()))
        raise_lib();
    return {image, T};
}

// need = (faces_opacity, vert_attrs, face_scale, bary) -> those four gradients, None where not asked for; grad_image
// [B,C,H,W] / grad_T [B,1,H,W]: None = zero
py::tuple composite_fragments_backward(In face, In bary, In faces, In faces_opacity, In vert_attrs, const std::optional<at::Tensor>& face_scale,
                                       const std::optional<at::Tensor>& grad_image, const std::optional<at::Tensor>& grad_T,
                                       const std::array<bool, 4>& need) {
    const ShadeArgs a = shade_args(face, bary, faces, faces_opacity, vert_attrs, face_scale);
    c10::DeviceGuard guard(a.dev);
    if (need[2] && !face_scale) err("composite_fragments_backward: the gradient of face_scale without face_scale");
    const auto [gi, gt] = upstreams(a, a.C, grad_image, grad_T);
    at::Tensor d_op = grad_if(need[0], {a.F}, a.dev), d_attrs = grad_if(need[1], {a.P, a.C}, a.dev);
    at::Tensor d_scale = grad_if(need[2], {a.B, a.F}, a.dev), d_bary = grad_if(need[3], {a.B, a.K, 2, a.H, a.W}, a.dev);
    if (g_abi.composite_fragments_backward(a.B, a.K, a.H, a.W, a.P, a.F, a.C, mptr<const int32_t>(a.face), mptr<const float>(a.bary),
                                           mptr<const int32_t>(a.corners), mptr<const float>(a.opacity), mptr<const float>(a.attrs), a.scale_ptr(),
                                           in_ptr(gi), in_ptr(gt), out_ptr(d_op), out_ptr(d_attrs), out_ptr(d_scale), out_ptr(d_bary), a.stream()))
        raise_lib();
    return py::make_tuple(or_none(d_op), or_none(d_attrs), or_none(d_scale), or_none(d_bary));
}

// -- composite_texture: a bilinear texture at per-corner UVs
struct TextureArgs : ListArgs { at::Tensor uvs, tex; int64_t Pu = 0, C = 0, Ht = 0, Wt = 0; int wrap = 0; };

TextureArgs texture_args(In face, In bary, In uv_faces, In faces_opacity, In vert_uvs, In texture, const std::optional<at::Tensor>& face_scale,
                         int wrap) {
    built(g_abi.composite_texture, "dmr_composite_texture");
    TextureArgs a;
    list_dims(a, "composite_texture", "uv_faces", face, bary, uv_faces, faces_opacity);
    if (vert_uvs.dim() != 2 || vert_uvs.size(1) != 2) err("vert_uvs must have dimensions (num_uvs, 2)");
    if (texture.dim() != 3) err("texture must have dimensions (Ht, Wt, C)");
    a.Pu = vert_uvs.size(0); a.Ht = texture.size(0); a.Wt = texture.size(1); a.C = texture.size(2); a.wrap = wrap;
    check_k(a);
    check_c(a, a.C, 32);
    if (a.Ht < 1 || a.Wt < 1 || a.Ht >= ((int64_t)1 << 31) || a.Wt >= ((int64_t)1 << 31)) err("composite_texture: the texture must have at least one texel");
    check_not_empty(a);
    if (wrap != 0 && wrap != 1) err("composite_texture: wrap must be 0 (clamp) or 1 (repeat), got " + std::to_string(wrap));
    list_finish(a, face_scale, {{vert_uvs, "vert_uvs", a.uvs}, {texture, "texture", a.tex}});
    return a;
}

// -> (image [B,C,H,W], T [B,1,H,W])
std::tuple<at::Tensor, at::Tensor> composite_texture(In face, In bary, In uv_faces, In faces_opacity, In vert_uvs, In texture,
                                                     const std::optional<at::Tensor>& face_scale, int wrap) {
    const TextureArgs a = texture_args(face, bary, uv_faces, faces_opacity, vert_uvs, texture, face_scale, wrap);
    c10::DeviceGuard guard(a.dev);
    auto [image, T] = image_and_T(a, a.C);
    if (g_abi.composite_texture(a.B, a.K, a.H, a.W, a.Pu, a.F, a.C, a.Ht, a.Wt, a.wrap, mptr<const int32_t>(a.face), mptr<const float>(a.bary),
                                mptr<const int32_t>(a.corners), mptr<const float>(a.opacity), mptr<const float>(a.uvs), mptr<const float>(a.tex),
                                a.scale_ptr(), mptr<float>(image), mptr<float>(T), a.stream()))
        raise_lib();
    return {image, T};
}

// need = (faces_opacity, vert_uvs, texture, face_scale, bary) -> those five gradients, None where not asked for; grad_image
// [B,C,H,W] / grad_T [B,1,H,W]: None = zero
py::tuple composite_texture_backward(In face, In bary, In uv_faces, In faces_opacity, In vert_uvs, In texture,
                                     const std::optional<at::Tensor>& face_scale, int wrap, const std::optional<at::Tensor>& grad_image,
                                     const std::optional<at::Tensor>& grad_T, const std::array<bool, 5>& need) {
    const TextureArgs a = texture_args(face, bary, uv_faces, faces_opacity, vert_uvs, texture, face_scale, wrap);
    c10::DeviceGuard guard(a.dev);
    if (need[3] && !face_scale) err("composite_texture_backward: the gradient of face_scale without face_scale");
    const auto [gi, gt] = upstreams(a, a.C, grad_image, grad_T);
    at::Tensor d_op = grad_if(need[0], {a.F}, a.dev), d_uvs = grad_if(need[1], {a.Pu, 2}, a.dev), d_tex = grad_if(need[2], {a.Ht, a.Wt, a.C}, a.dev);
    at::Tensor d_scale = grad_if(need[3], {a.B, a.F}, a.dev), d_bary = grad_if(need[4], {a.B, a.K, 2, a.H, a.W}, a.dev);
    if (g_abi.composite_texture_backward(a.B, a.K, a.H, a.W, a.Pu, a.F, a.C, a.Ht, a.Wt, a.wrap, mptr<const int32_t>(a.face),
                                         mptr<const float>(a.bary), mptr<const int32_t>(a.corners), mptr<const float>(a.opacity),
                                         mptr<const float>(a.uvs), mptr<const float>(a.tex), a.scale_ptr(), in_ptr(gi), in_ptr(gt),
                                         out_ptr(d_op), out_ptr(d_uvs), out_ptr(d_tex), out_ptr(d_scale), out_ptr(d_bary), a.stream()))
        raise_lib();
    return py::make_tuple(or_none(d_op), or_none(d_uvs), or_none(d_tex), or_none(d_scale), or_none(d_bary));
}

// -- face_visibility: per-face visibility and coverage.  It reads the face ids and the opacities alone.
struct VisArgs : Lists { at::Tensor opacity, weight; int64_t F = 0; };  // weight: undefined = none

VisArgs vis_args(In face, In faces_opacity, const std::optional<at::Tensor>& pixel_weight) {
    built(g_abi.face_visibility, "dmr_face_visibility");
    VisArgs a;
    lists_begin(a, "face_visibility", face);
    check_k(a);
    check_not_empty(a);
    a.F = check_opacity(faces_opacity);
    if (pixel_weight && (pixel_weight->dim() != 3 || pixel_weight->size(0) != a.B || pixel_weight->size(1) != a.H || pixel_weight->size(2) != a.W))
        err("pixel_weight must have dimensions (B, H, W) of pix_to_face's B, H, W");
    same_device(a, faces_opacity, "faces_opacity");
    same_device(a, pixel_weight, "pixel_weight");
    a.face = i32(face, "pix_to_face"); a.opacity = f32(faces_opacity, "faces_opacity");
    if (pixel_weight) a.weight = f32(*pixel_weight, "pixel_weight");
    return a;
}

// -> (vis [B,F], max_weight [B,F], pixels i32 [B,F]); the last two None without coverage
py::tuple face_visibility(In face, In faces_opacity, const std::optional<at::Tensor>& pixel_weight, bool coverage) {
    const VisArgs a = vis_args(face, faces_opacity, pixel_weight);
    c10::DeviceGuard guard(a.dev);
    at::Tensor vis = at::empty({a.B, a.F}, f32_on(a.dev)), max_weight, pixels;
    if (coverage) {
        max_weight = at::empty({a.B, a.F}, f32_on(a.dev));
        pixels = at::empty({a.B, a.F}, at::TensorOptions().dtype(at::kInt).device(a.dev));
    }
    // (F == 0: the three are empty and their pointers null, which the call takes: it has nothing to write)
    if (a.F > 0 && g_abi.face_visibility(a.B, a.K, a.H, a.W, a.F, mptr<const int32_t>(a.face), mptr<const float>(a.opacity), in_ptr(a.weight),
                                         mptr<float>(vis), out_ptr(max_weight), coverage ? mptr<int32_t>(pixels) : nullptr, a.stream()))
        raise_lib();
    return py::make_tuple(vis, or_none(max_weight), or_none(pixels));
}

// need = (faces_opacity, pixel_weight) -> those two gradients, None where not asked for; grad_vis [B,F]
py::tuple face_visibility_backward(In face, In faces_opacity, const std::optional<at::Tensor>& pixel_weight, In grad_vis,
                                   const std::array<bool, 2>& need) {
    const VisArgs a = vis_args(face, faces_opacity, pixel_weight);
    c10::DeviceGuard guard(a.dev);
    if (need[1] && !pixel_weight) err("face_visibility_backward: the gradient of pixel_weight without pixel_weight");
    if (grad_vis.dim() != 2 || grad_vis.size(0) != a.B || grad_vis.size(1) != a.F || grad_vis.device() != a.dev)
        err("grad_vis must have dimensions (B, num_faces) on the device of pix_to_face");
    const at::Tensor gv = f32(grad_vis, "grad_vis");
    at::Tensor d_op = grad_if(need[0], {a.F}, a.dev), d_pw = grad_if(need[1], {a.B, a.H, a.W}, a.dev);
    if (g_abi.face_visibility_backward(a.B, a.K, a.H, a.W, a.F, mptr<const int32_t>(a.face), mptr<const float>(a.opacity), in_ptr(a.weight),
                                       mptr<const float>(gv), out_ptr(d_op), out_ptr(d_pw), a.stream()))
        raise_lib();
    return py::make_tuple(or_none(d_op), or_none(d_pw));
}

// -- interpolate_fragments / composite_values, the two ends of a deferred shader on [B,K,C,H,W] planes, and pack_slots /
// interpolate_packed / composite_values_packed, the same on [N,C] rows: row [B,K,H,W] and n_used [1] come from pack_slots.  A
// packed argument block is the dense one and PackedRows; the two builders of a pair share the checks of the pair's own tensors.
struct InterpArgs : Lists { at::Tensor bary, faces, attrs; int64_t F = 0, P = 0, C = 0; };
struct ValuesArgs : Lists, Blend { at::Tensor values; int64_t C = 0; };
struct PackedRows { at::Tensor row, n_used; int64_t N = 0; };
struct PackedInterpArgs : InterpArgs, PackedRows {};
struct PackedValuesArgs : ValuesArgs, PackedRows {};

// face [B,K,H,W] with K in 1..32 and at least one pixel; row (if given) of its shape, n_used (if given) one element, on its device
void packed_lists(Lists& a, PackedRows& r, const char* call, In face, const at::Tensor* row, const at::Tensor* n_used) {
    built(g_abi.pack_slots, "dmr_pack_slots");
    lists_begin(a, call, face);
    if (row && (row->dim() != 4 || row->sizes() != face.sizes())) err("row must have the dimensions (B, K, H, W) of pix_to_face");
    if (n_used && n_used->numel() != 1) err("n_used must have one element");
    check_k(a);
    check_not_empty(a);
    if (a.B * a.K * a.H * a.W >= ((int64_t)1 << 31)) err(std::string(call) + ": B K H W must be below 2^31");
    if (row) same_device(a, *row, "row");
    if (n_used) same_device(a, *n_used, "n_used");
    a.face = i32(face, "pix_to_face");
    if (row) r.row = i32(*row, "row");
    if (n_used) r.n_used = i32(*n_used, "n_used");
}
void check_rows(const Lists& a, int64_t N) {
    if (N < 0 || N >= ((int64_t)1 << 31)) err(std::string(a.call) + ": rows must be in 0..2^31 - 1, got " + std::to_string(N));
}

// an interpolate call's own tensors: their shapes ...
void interp_shapes(InterpArgs& a, In bary, In faces, In vert_attrs) {
    check_bary(a, bary);
    a.F = check_corners(faces, "faces");
    check_attrs(vert_attrs, a.P, a.C);
}
// ... and, after the unit's size checks, one device, then dtypes (a packed call's face is contiguous already: packed_lists)
void interp_finish(InterpArgs& a, In face, In bary, In faces, In vert_attrs) {
    same_device(a, bary, "bary"); same_device(a, faces, "faces"); same_device(a, vert_attrs, "vert_attrs");
    if (!a.face.defined()) a.face = i32(face, "pix_to_face");
    a.bary = f32(bary, "bary"); a.faces = i32(faces, "faces"); a.attrs = f32(vert_attrs, "vert_attrs");
}
// what a composite_values call does after its size checks: face_scale's shape, one device, then dtypes
void values_finish(ValuesArgs& a, In face, In faces_opacity, In values, const std::optional<at::Tensor>& face_scale) {
    check_scale(a, a.F, face_scale);
    same_device(a, faces_opacity, "faces_opacity"); same_device(a, values, "values"); same_device(a, face_scale, "face_scale");
    if (!a.face.defined()) a.face = i32(face, "pix_to_face");
    a.opacity = f32(faces_opacity, "faces_opacity"); a.values = f32(values, "values");
    if (face_scale) a.scale = f32(*face_scale, "face_scale");
}

InterpArgs interp_args(In face, In bary, In faces, In vert_attrs) {
    built(g_abi.interpolate_fragments, "dmr_interpolate_fragments");
    InterpArgs a;
    lists_begin(a, "interpolate_fragments", face);
    interp_shapes(a, bary, faces, vert_attrs);
    check_k(a);
    check_c(a, a.C, 256);
    check_not_empty(a);
    interp_finish(a, face, bary, faces, vert_attrs);
    return a;
}

PackedInterpArgs packed_interp_args(In face, In bary, In row, In n_used, In faces, In vert_attrs, int64_t N) {
    PackedInterpArgs a;
    packed_lists(a, a, "interpolate_packed", face, &row, &n_used);
    interp_shapes(a, bary, faces, vert_attrs);
    a.N = N;
    check_c(a, a.C, 256);
    check_rows(a, N);
    interp_finish(a, face, bary, faces, vert_attrs);
    return a;
}

ValuesArgs values_args(In face, In faces_opacity, In values, const std::optional<at::Tensor>& face_scale) {
    built(g_abi.composite_values, "dmr_composite_values");
    ValuesArgs a;
    lists_begin(a, "composite_values", face);
    a.F = check_opacity(faces_opacity);
    if (values.dim() != 5 || values.size(0) != a.B || values.size(1) != a.K || values.size(3) != a.H || values.size(4) != a.W)
        err("values must have dimensions (B, K, C, H, W) of pix_to_face's B, K, H, W");
    a.C = values.size(2);
    check_k(a);
    check_c(a, a.C, 256);
    check_not_empty(a);
    values_finish(a, face, faces_opacity, values, face_scale);
    return a;
}

PackedValuesArgs packed_values_args(In face, In row, const at::Tensor* n_used, In faces_opacity, In values, const std::optional<at::Tensor>& face_scale) {
    PackedValuesArgs a;
    packed_lists(a, a, "composite_values_packed", face, &row, n_used);
    a.F = check_opacity(faces_opacity);
    if (values.dim() != 2) err("values must have dimensions (rows, C)");
    a.N = values.size(0); a.C = values.size(1);
    check_c(a, a.C, 256);
    check_rows(a, a.N);
    values_finish(a, face, faces_opacity, values, face_scale);
    return a;
}

// -> out [B,K,C,H,W]
at::Tensor interpolate_fragments(In face, In bary, In faces, In vert_attrs) {
    const InterpArgs a = interp_args(face, bary, faces, vert_attrs);
    c10::DeviceGuard guard(a.dev);
    at::Tensor out = at::empty({a.B, a.K, a.C, a.H, a.W}, f32_on(a.dev));
    if (g_abi.interpolate_fragments(a.B, a.K, a.H, a.W, a.P, a.F, a.C, mptr<const int32_t>(a.face), mptr<const float>(a.bary),
                                    mptr<const int32_t>(a.faces), mptr<const float>(a.attrs), mptr<float>(out), a.stream()))
        raise_lib();
    return out;
}

// need = (vert_attrs, bary) -> those two gradients, None where not asked for; grad_out [B,K,C,H,W]
py::tuple interpolate_fragments_backward(In face, In bary, In faces, In vert_attrs, In grad_out, const std::array<bool, 2>& need) {
    const InterpArgs a = interp_args(face, bary, faces, vert_attrs);
    c10::DeviceGuard guard(a.dev);
    if (grad_out.dim() != 5 || grad_out.size(0) != a.B || grad_out.size(1) != a.K || grad_out.size(2) != a.C || grad_out.size(3) != a.H ||
        grad_out.size(4) != a.W || grad_out.device() != a.dev)
        err("grad_out must have dimensions (B, K, C, H, W) on the device of pix_to_face");
    const at::Tensor go = f32(grad_out, "grad_out");
    at::Tensor d_attrs = grad_if(need[0], {a.P, a.C}, a.dev), d_bary = grad_if(need[1], {a.B, a.K, 2, a.H, a.W}, a.dev);
    if (g_abi.interpolate_fragments_backward(a.B, a.K, a.H, a.W, a.P, a.F, a.C, mptr<const int32_t>(a.face), mptr<const float>(a.bary),
                                             mptr<const int32_t>(a.faces), mptr<const float>(a.attrs), mptr<const float>(go),
                                             out_ptr(d_attrs), out_ptr(d_bary), a.stream()))
        raise_lib();
    return py::make_tuple(or_none(d_attrs), or_none(d_bary));
}

// -> (image [B,C,H,W], T [B,1,H,W])
std::tuple<at::Tensor, at::Tensor> composite_values(In face, In faces_opacity, In values, const std::optional<at::Tensor>& face_scale) {
    const ValuesArgs a = values_args(face, faces_opacity, values, face_scale);
    c10::DeviceGuard guard(a.dev);
    auto [image, T] = image_and_T(a, a.C);
    if (g_abi.composite_values(a.B, a.K, a.H, a.W, a.F, a.C, mptr<const int32_t>(a.face), in_ptr(a.opacity), mptr<const float>(a.values),
                               a.scale_ptr(), mptr<float>(image), mptr<float>(T), a.stream()))
        raise_lib();
    return {image, T};
}

// need = (faces_opacity, values, face_scale) -> those three gradients, None where not asked for; grad_image [B,C,H,W] /
// grad_T [B,1,H,W]: None = zero
py::tuple composite_values_backward(In face, In faces_opacity, In values, const std::optional<at::Tensor>& face_scale,
                                    const std::optional<at::Tensor>& grad_image, const std::optional<at::Tensor>& grad_T,
                                    const std::array<bool, 3>& need) {
    const ValuesArgs a = values_args(face, faces_opacity, values, face_scale);
    c10::DeviceGuard guard(a.dev);
    if (need[2] && !face_scale) err("composite_values_backward: the gradient of face_scale without face_scale");
    const auto [gi, gt] = upstreams(a, a.C, grad_image, grad_T);
    at::Tensor d_op = grad_if(need[0], {a.F}, a.dev), d_values = grad_if(need[1], {a.B, a.K, a.C, a.H, a.W}, a.dev);
    at::Tensor d_scale = grad_if(need[2], {a.B, a.F}, a.dev);
    if (g_abi.composite_values_backward(a.B, a.K, a.H, a.W, a.F, a.C, mptr<const int32_t>(a.face), in_ptr(a.opacity),
                                        mptr<const float>(a.values), a.scale_ptr(), in_ptr(gi), in_ptr(gt), out_ptr(d_op),
                                        out_ptr(d_values), out_ptr(d_scale), a.stream()))
        raise_lib();
    return py::make_tuple(or_none(d_op), or_none(d_values), or_none(d_scale));
}

// -> (row [B,K,H,W] int32, n_used [1] int32); a used slot (face id in [0, F)) whose row would be >= capacity gets -1
std::tuple<at::Tensor, at::Tensor> pack_slots(In face, int64_t F, int64_t capacity) {
    Lists a;
    PackedRows none;
    packed_lists(a, none, "pack_slots", face, nullptr, nullptr);
    if (F < 0 || F >= ((int64_t)1 << 31)) err("pack_slots: F must be in 0..2^31 - 1, got " + std::to_string(F));
    if (capacity < 0) err("pack_slots: capacity must not be negative, got " + std::to_string(capacity));
    c10::DeviceGuard guard(a.dev);
    const at::TensorOptions i32_on = at::TensorOptions().dtype(at::kInt).device(a.dev);
    at::Tensor row = at::empty({a.B, a.K, a.H, a.W}, i32_on), n_used = at::empty({1}, i32_on);
    if (g_abi.pack_slots(a.B, a.K, a.H, a.W, (int)F, (int)std::min<int64_t>(capacity, INT32_MAX), mptr<const int32_t>(a.face),
                         mptr<int32_t>(row), mptr<int32_t>(n_used), a.stream()))
        raise_lib();
    return {row, n_used};
}
// -> out [N,C]
at::Tensor interpolate_packed(In face, In bary, In row, In n_used, In faces, In vert_attrs, int64_t N) {
    const PackedInterpArgs a = packed_interp_args(face, bary, row, n_used, faces, vert_attrs, N);
    c10::DeviceGuard guard(a.dev);
    at::Tensor out = at::empty({a.N, a.C}, f32_on(a.dev));
    if (g_abi.interpolate_packed(a.B, a.K, a.H, a.W, a.P, a.F, a.C, a.N, mptr<const int32_t>(a.face), mptr<const float>(a.bary),
                                 mptr<const int32_t>(a.row), mptr<const int32_t>(a.n_used), mptr<const int32_t>(a.faces),
                                 mptr<const float>(a.attrs), mptr<float>(out), a.stream()))
        raise_lib();
    return out;
}

// need = (vert_attrs, bary) -> those two gradients, None where not asked for; grad_out [N,C]
py::tuple interpolate_packed_backward(In face, In bary, In row, In n_used, In faces, In vert_attrs, In grad_out, const std::array<bool, 2>& need) {
    const PackedInterpArgs a = packed_interp_args(face, bary, row, n_used, faces, vert_attrs, grad_out.dim() == 2 ? grad_out.size(0) : -1);
    c10::DeviceGuard guard(a.dev);
    if (grad_out.dim() != 2 || grad_out.size(1) != a.C || grad_out.device() != a.dev) err("grad_out must have dimensions (rows, C) on the device of pix_to_face");
    const at::Tensor go = f32(grad_out, "grad_out");
    at::Tensor d_attrs = grad_if(need[0], {a.P, a.C}, a.dev), d_bary = grad_if(need[1], {a.B, a.K, 2, a.H, a.W}, a.dev);
    if (g_abi.interpolate_packed_backward(a.B, a.K, a.H, a.W, a.P, a.F, a.C, a.N, mptr<const int32_t>(a.face), mptr<const float>(a.bary),
                                          mptr<const int32_t>(a.row), mptr<const int32_t>(a.n_used), mptr<const int32_t>(a.faces),
                                          mptr<const float>(a.attrs), mptr<const float>(go), out_ptr(d_attrs), out_ptr(d_bary), a.stream()))
        raise_lib();
    return py::make_tuple(or_none(d_attrs), or_none(d_bary));
}

// -> (image [B,C,H,W], T [B,1,H,W])
std::tuple<at::Tensor, at::Tensor> composite_values_packed(In face, In row, In faces_opacity, In values, const std::optional<at::Tensor>& face_scale) {
    const PackedValuesArgs a = packed_values_args(face, row, nullptr, faces_opacity, values, face_scale);
    c10::DeviceGuard guard(a.dev);
    auto [image, T] = image_and_T(a, a.C);
    if (g_abi.composite_values_packed(a.B, a.K, a.H, a.W, a.F, a.C, a.N, mptr<const int32_t>(a.face), mptr<const int32_t>(a.row), in_ptr(a.opacity),
                                      in_ptr(a.values), a.scale_ptr(), mptr<float>(image), mptr<float>(T), a.stream()))
        raise_lib();
    return {image, T};
}

// need = (faces_opacity, values, face_scale) -> those three gradients, None where not asked for; grad_image [B,C,H,W] /
// grad_T [B,1,H,W]: None = zero
py::tuple composite_values_packed_backward(In face, In row, In n_used, In faces_opacity, In values, const std::optional<at::Tensor>& face_scale,
                                           const std::optional<at::Tensor>& grad_image, const std::optional<at::Tensor>& grad_T,
                                           const std::array<bool, 3>& need) {
    const PackedValuesArgs a = packed_values_args(face, row, &n_used, faces_opacity, values, face_scale);
    c10::DeviceGuard guard(a.dev);
    if (need[2] && !face_scale) err("composite_values_packed_backward: the gradient of face_scale without face_scale");
    const auto [gi, gt] = upstreams(a, a.C, grad_image, grad_T);
    at::Tensor d_op = grad_if(need[0], {a.F}, a.dev), d_values = grad_if(need[1], {a.N, a.C}, a.dev);
    at::Tensor d_scale = grad_if(need[2], {a.B, a.F}, a.dev);
    if (g_abi.composite_values_packed_backward(a.B, a.K, a.H, a.W, a.F, a.C, a.N, mptr<const int32_t>(a.face), mptr<const int32_t>(a.row),
                                               mptr<const int32_t>(a.n_used), in_ptr(a.opacity), in_ptr(a.values), a.scale_ptr(), in_ptr(gi),
                                               in_ptr(gt), out_ptr(d_op), out_ptr(d_values), out_ptr(d_scale), a.stream()))
        raise_lib();
    return py::make_tuple(or_none(d_op), or_none(d_values), or_none(d_scale));
}

// -- surface_packed: the surface frame of packed rows (dmesh_renderer_amd_surface.h).  The interpolate_packed argument block with
// attrs = verts [P,3], and origin [B,3]: one camera centre per view of the lists; its own builder, so that every message names
// this call and its tensors.
struct SurfaceArgs : PackedInterpArgs { at::Tensor origin; };

SurfaceArgs surface_args(In face, In bary, In row, In n_used, In faces, In verts, In origin, int64_t N) {
    built(g_abi.surface_packed, "dmr_surface_packed");
    SurfaceArgs a;
    packed_lists(a, a, "surface_packed", face, &row, &n_used);
    check_bary(a, bary);
    a.F = check_corners(faces, "faces");
    if (verts.dim() != 2 || verts.size(1) != 3) err("verts must have dimensions (num_points, 3)");
    if (origin.dim() != 2 || origin.size(0) != a.B || origin.size(1) != 3) err("origin must have dimensions (B, 3) of pix_to_face's B");
    a.P = verts.size(0); a.C = 3; a.N = N;
    check_rows(a, N);
    same_device(a, bary, "bary"); same_device(a, faces, "faces"); same_device(a, verts, "verts"); same_device(a, origin, "origin");
    a.bary = f32(bary, "bary"); a.faces = i32(faces, "faces"); a.attrs = f32(verts, "verts"); a.origin = f32(origin, "origin");
    return a;
}

// -> (hit, normal, reflect), each [N,3]
std::tuple<at::Tensor, at::Tensor, at::Tensor> surface_packed(In face, In bary, In row, In n_used, In faces, In verts, In origin, int64_t N) {
    const SurfaceArgs a = surface_args(face, bary, row, n_used, faces, verts, origin, N);
    c10::DeviceGuard guard(a.dev);
    at::Tensor hit = at::empty({a.N, 3}, f32_on(a.dev)), normal = at::empty({a.N, 3}, f32_on(a.dev)), reflect = at::empty({a.N, 3}, f32_on(a.dev));
    if (g_abi.surface_packed(a.B, a.K, a.H, a.W, a.P, a.F, a.N, mptr<const int32_t>(a.face), mptr<const float>(a.bary), mptr<const int32_t>(a.row),
                             mptr<const int32_t>(a.n_used), mptr<const int32_t>(a.faces), mptr<const float>(a.attrs), mptr<const float>(a.origin),
                             mptr<float>(hit), mptr<float>(normal), mptr<float>(reflect), a.stream()))
        raise_lib();
    return {hit, normal, reflect};
}

// need = (verts, bary, origin) -> those three gradients, None where not asked for; grad_hit / grad_normal / grad_reflect [N,3]:
// None = zero (N: the rows of those that arrive, which must agree)
py::tuple surface_packed_backward(In face, In bary, In row, In n_used, In faces, In verts, In origin, const std::optional<at::Tensor>& grad_hit,
                                  const std::optional<at::Tensor>& grad_normal, const std::optional<at::Tensor>& grad_reflect,
                                  const std::array<bool, 3>& need) {
    int64_t N = -1;
    for (const auto* g : {&grad_hit, &grad_normal, &grad_reflect}) {
        if (!*g) continue;
        if ((*g)->dim() != 2 || (*g)->size(1) != 3 || (N >= 0 && (*g)->size(0) != N)) err("the upstream gradients must have dimensions (rows, 3), the same rows");
        N = (*g)->size(0);
    }
    if (N < 0) err("surface_packed_backward: no upstream gradient");
    const SurfaceArgs a = surface_args(face, bary, row, n_used, faces, verts, origin, N);
    c10::DeviceGuard guard(a.dev);
    at::Tensor gs[3];
    const std::optional<at::Tensor>* in[3] = {&grad_hit, &grad_normal, &grad_reflect};
    for (int i = 0; i < 3; i++) {
        if (!*in[i]) continue;
        same_device(a, **in[i], "an upstream gradient");
        gs[i] = f32(**in[i], "an upstream gradient");
    }
    at::Tensor d_verts = grad_if(need[0], {a.P, 3}, a.dev), d_bary = grad_if(need[1], {a.B, a.K, 2, a.H, a.W}, a.dev);
    at::Tensor d_origin = grad_if(need[2], {a.B, 3}, a.dev);
    if (g_abi.surface_packed_backward(a.B, a.K, a.H, a.W, a.P, a.F, a.N, mptr<const int32_t>(a.face), mptr<const float>(a.bary),
                                      mptr<const int32_t>(a.row), mptr<const int32_t>(a.n_used), mptr<const int32_t>(a.faces),
                                      mptr<const float>(a.attrs), mptr<const float>(a.origin), in_ptr(gs[0]), in_ptr(gs[1]), in_ptr(gs[2]),
                                      out_ptr(d_verts), out_ptr(d_bary), out_ptr(d_origin), a.stream()))
        raise_lib();
    return py::make_tuple(or_none(d_verts), or_none(d_bary), or_none(d_origin));
}

// -- The row units (mlp_rows, hashgrid_rows, sh_rows, envmap_rows) start from x [N,C] on a HIP device and an optional count n_rows [1]: RowArgs.
// A unit's argument block extends it, and its builder calls the named checks below in the unit's order, which is fragments.py's:
// shapes, sizes, one device, dtypes.
struct RowArgs {
    at::Tensor x, n_rows;  // n_rows undefined: none
    int64_t N = 0;
    c10::Device dev{c10::kCPU};
    const char* call = "";  // what the unit's own messages start with: "mlp_rows", ...
    void* stream() const { return stream_on(dev); }
    const int32_t* rows_ptr() const { return n_rows.defined() ? mptr<const int32_t>(n_rows) : nullptr; }
};
// fn: the unit's forward in g_abi, dmr_<call>; then the device, x [N, cols] (cols 0: any width; cols_name: what the message calls it) and N
template <class Fn>
void rows_begin(RowArgs& a, const char* call, Fn fn, In x, int64_t cols, const char* cols_name) {
    built(fn, (std::string("dmr_") + call).c_str());
    a.call = call; a.dev = hip_device_of(x);
    if (x.dim() != 2 || (cols && x.size(1) != cols)) err(std::string("x must have dimensions (rows, ") + cols_name + ")");
    a.N = x.size(0);
}
void check_row_count(const RowArgs& a) { if (a.N >= ((int64_t)1 << 31)) err(std::string(a.call) + ": rows must be below 2^31"); }
void check_n_rows(const std::optional<at::Tensor>& n_rows) { if (n_rows && n_rows->numel() != 1) err("n_rows must have one element"); }
void on_device_of_x(const RowArgs& a, In t, const std::string& what) { if (t.device() != a.dev) err(what + " must be on the device of x"); }
void on_device_of_x(const RowArgs& a, const std::optional<at::Tensor>& t, const std::string& what) { if (t) on_device_of_x(a, *t, what); }
// where the device checks end and the dtypes begin (n_rows is the last tensor of the one, x the first of the other), and where those end
void rows_devices_end(RowArgs& a, In x, const std::optional<at::Tensor>& n_rows) { on_device_of_x(a, n_rows, "n_rows"); a.x = f32(x, "x"); }
void rows_finish(RowArgs& a, const std::optional<at::Tensor>& n_rows) { if (n_rows) a.n_rows = i32(*n_rows, "n_rows"); }
// a backward's upstream [N, cols]; cols_name: "Cout", "L * F", "degree^2"
void check_grad_out(const RowArgs& a, In grad_out, int64_t cols, const char* cols_name) {
    if (grad_out.dim() != 2 || grad_out.size(0) != a.N || grad_out.size(1) != cols || grad_out.device() != a.dev)
        err(std::string("grad_out must have dimensions (rows, ") + cols_name + ") on the device of x");
}

// -- mlp_rows: a small MLP over [N,Cin] rows (dmesh_renderer_amd_mlp.h).  weights = (W_in [Hd,Cin], [W_mid [Hd,Hd],] W_out [Cout,Hd]),
// biases = one per weight, each a tensor or None.
using OptTensors = std::vector<std::optional<at::Tensor>>;
struct MlpArgs : RowArgs {
    std::vector<at::Tensor> w, b;  // b[l] undefined: no bias
    int64_t Cin = 0, Hd = 0, Cout = 0;
    int nh = 0, act = 0, oact = 0;
    const float* wp(size_t l) const { return mptr<const float>(w[l]); }
    const float* bp(size_t l) const { return b[l].defined() ? mptr<const float>(b[l]) : nullptr; }
    const float* mid_w() const { return nh == 2 ? wp(1) : nullptr; }
    const float* mid_b() const { return nh == 2 ? bp(1) : nullptr; }
};

MlpArgs mlp_args(In x, const std::vector<at::Tensor>& weights, const OptTensors& biases, int64_t act, int64_t oact,
                 const std::optional<at::Tensor>& n_rows) {
    MlpArgs a;
    rows_begin(a, "mlp_rows", g_abi.mlp_rows, x, 0, "Cin");
    if (weights.size() != 2 && weights.size() != 3) err("mlp_rows: 2 or 3 weights (1 or 2 hidden layers), got " + std::to_string(weights.size()));
    if (biases.size() != weights.size()) err("mlp_rows: one bias (or None) per weight");
    a.nh = (int)weights.size() - 1;
    a.Cin = x.size(1);
    for (const at::Tensor& w : weights)
        if (w.dim() != 2) err("mlp_rows: every weight must have dimensions (out, in)");
    a.Hd = weights[0].size(0); a.Cout = weights.back().size(0);
    if (a.Hd != 16 && a.Hd != 32 && a.Hd != 64) err("mlp_rows: the hidden width must be 16, 32 or 64, got " + std::to_string(a.Hd));
    if (a.Cin < 1 || a.Cin > 64) err("mlp_rows: Cin must be in 1..64, got " + std::to_string(a.Cin));
    if (a.Cout < 1 || a.Cout > 16) err("mlp_rows: Cout must be in 1..16, got " + std::to_string(a.Cout));
    check_row_count(a);
    int64_t in = a.Cin;
    for (size_t l = 0; l < weights.size(); l++) {
        const int64_t out = l + 1 == weights.size() ? a.Cout : a.Hd;
        if (weights[l].size(0) != out || weights[l].size(1) != in) err("mlp_rows: weight " + std::to_string(l) + " must have dimensions (" + std::to_string(out) + ", " + std::to_string(in) + ")");
        if (biases[l] && (biases[l]->dim() != 1 || biases[l]->size(0) != out)) err("mlp_rows: bias " + std::to_string(l) + " must have dimensions (" + std::to_string(out) + ",)");
        in = out;
    }
    if (act < 0 || act > 1 || oact < 0 || oact > 1) err("mlp_rows: bad activation");
    check_n_rows(n_rows);
    const char* both = "mlp_rows: the weights and biases";
    for (size_t l = 0; l < weights.size(); l++) { on_device_of_x(a, weights[l], both); on_device_of_x(a, biases[l], both); }
    rows_devices_end(a, x, n_rows);
    for (size_t l = 0; l < weights.size(); l++) {
        a.w.push_back(f32(weights[l], "weight"));
        a.b.push_back(biases[l] ? f32(*biases[l], "bias") : at::Tensor());
    }
    rows_finish(a, n_rows);
    a.act = (int)act; a.oact = (int)oact;
    return a;
}

// -> y [N,Cout]
at::Tensor mlp_rows(In x, const std::vector<at::Tensor>& weights, const OptTensors& biases, int64_t act, int64_t oact,
                    const std::optional<at::Tensor>& n_rows) {
    const MlpArgs a = mlp_args(x, weights, biases, act, oact, n_rows);
    c10::DeviceGuard guard(a.dev);
    at::Tensor y = at::empty({a.N, a.Cout}, f32_on(a.dev));
    if (g_abi.mlp_rows((int)a.N, (int)a.Cin, (int)a.Hd, (int)a.Cout, a.nh, a.act, a.oact, mptr<const float>(a.x), a.wp(0), a.bp(0), a.mid_w(),
                       a.mid_b(), a.wp(a.nh), a.bp(a.nh), a.rows_ptr(), mptr<float>(y), a.stream()))
        raise_lib();
    return y;
}

// need_x, need_w[l], need_b[l] -> (dL_dx, [dL_dW_l], [dL_db_l]), None where not asked for; grad_out [N,Cout].  The scratch of
// the weight-gradient reduction comes from PyTorch's allocator (DMR_MLP_SCRATCH_FLOATS), only when such a gradient is wanted.
py::tuple mlp_rows_backward(In x, const std::vector<at::Tensor>& weights, const OptTensors& biases, int64_t act, int64_t oact,
                            const std::optional<at::Tensor>& n_rows, In grad_out, bool need_x, const std::vector<bool>& need_w,
                            const std::vector<bool>& need_b) {
    const MlpArgs a = mlp_args(x, weights, biases, act, oact, n_rows);
    c10::DeviceGuard guard(a.dev);
    check_grad_out(a, grad_out, a.Cout, "Cout");
    if (need_w.size() != a.w.size() || need_b.size() != a.w.size()) err("mlp_rows_backward: one need flag per weight and per bias");
    const at::Tensor go = f32(grad_out, "grad_out");
    at::Tensor dx = grad_if(need_x, {a.N, a.Cin}, a.dev);
    std::vector<at::Tensor> dw(3), db(3);  // (in, mid, out)
    bool any = false;
    for (size_t l = 0; l < a.w.size(); l++) {
        const size_t slot = l + 1 == a.w.size() ? 2 : l;
        if (need_b[l] && !a.b[l].defined()) err("mlp_rows_backward: the gradient of a bias that was not given");
        dw[slot] = grad_if(need_w[l], a.w[l].sizes(), a.dev);
        db[slot] = grad_if(need_b[l], {a.w[l].size(0)}, a.dev);
        any = any || need_w[l] || need_b[l];
    }
    const int64_t scratch_floats = any ? DMR_MLP_SCRATCH_FLOATS(a.Hd, a.nh) : 0;
    at::Tensor scratch = any ? at::empty({scratch_floats}, f32_on(a.dev)) : at::Tensor();
    if (g_abi.mlp_rows_backward((int)a.N, (int)a.Cin, (int)a.Hd, (int)a.Cout, a.nh, a.act, a.oact, mptr<const float>(a.x), a.wp(0), a.bp(0),
                                a.mid_w(), a.mid_b(), a.wp(a.nh), a.bp(a.nh), a.rows_ptr(), mptr<const float>(go), out_ptr(dx), out_ptr(dw[0]),
                                out_ptr(db[0]), out_ptr(dw[1]), out_ptr(db[1]), out_ptr(dw[2]), out_ptr(db[2]), out_ptr(scratch), scratch_floats,
                                a.stream()))
        raise_lib();
    py::list gw, gb;
    for (size_t l = 0; l < a.w.size(); l++) {
        const size_t slot = l + 1 == a.w.size() ? 2 : l;
        gw.append(or_none(dw[slot])); gb.append(or_none(db[slot]));
    }
    return py::make_tuple(or_none(dx), gw, gb);
}

// -- hashgrid_rows: a multiresolution hash-grid encoding of [N,3] rows (dmesh_renderer_amd_hashgrid.h).  resolutions: the L
// levels' R_l (host integers); table [rows,F] with rows = what dmr_hashgrid_layout gives.
struct HashGridArgs : RowArgs {
    at::Tensor table;
    std::vector<int32_t> res;
    int64_t L = 0, F = 0, rows = 0;
    int log2_T = 0;
};

HashGridArgs hashgrid_args(In x, In table, const std::vector<int64_t>& resolutions, int64_t log2_T, const std::optional<at::Tensor>& n_rows) {
    HashGridArgs a;
    rows_begin(a, "hashgrid_rows", g_abi.hashgrid_rows, x, 3, "3");
    if (table.dim() != 2) err("table must have dimensions (rows, F)");
    a.L = (int64_t)resolutions.size(); a.F = table.size(1);
    if (a.L < 1 || a.L > DMR_HASHGRID_MAX_LEVELS) err("hashgrid_rows: 1 to 16 levels, got " + std::to_string(a.L));
    if (a.F != 1 && a.F != 2 && a.F != 4 && a.F != 8) err("hashgrid_rows: F must be 1, 2, 4 or 8, got " + std::to_string(a.F));
    if (a.L * a.F > DMR_HASHGRID_MAX_CHANNELS) err("hashgrid_rows: L * F must be at most 64, got " + std::to_string(a.L * a.F));
    if (log2_T < 4 || log2_T > 24) err("hashgrid_rows: log2_T must be in 4..24, got " + std::to_string(log2_T));
    for (int64_t r : resolutions) {
        if (r < 1 || r > 65536) err("hashgrid_rows: a resolution must be in 1..65536, got " + std::to_string(r));
        a.res.push_back((int32_t)r);
    }
    a.log2_T = (int)log2_T;
    std::vector<int64_t> offsets((size_t)a.L + 1);
    if (g_abi.hashgrid_layout((int)a.L, a.log2_T, a.res.data(), offsets.data())) raise_lib();
    a.rows = offsets.back();
    if (table.size(0) != a.rows) err("hashgrid_rows: table must have " + std::to_string(a.rows) + " rows, got " + std::to_string(table.size(0)));
    check_row_count(a);
    check_n_rows(n_rows);
    on_device_of_x(a, table, "hashgrid_rows: table");
    rows_devices_end(a, x, n_rows);
    a.table = f32(table, "table");
    rows_finish(a, n_rows);
    return a;
}

// -> y [N, L*F]
at::Tensor hashgrid_rows(In x, In table, const std::vector<int64_t>& resolutions, int64_t log2_T, const std::optional<at::Tensor>& n_rows) {
    const HashGridArgs a = hashgrid_args(x, table, resolutions, log2_T, n_rows);
    c10::DeviceGuard guard(a.dev);
    at::Tensor y = at::empty({a.N, a.L * a.F}, f32_on(a.dev));
    if (g_abi.hashgrid_rows((int)a.N, (int)a.L, (int)a.F, a.log2_T, a.res.data(), mptr<const float>(a.x), reinterpret_cast<const float*>(a.table.data_ptr()),
                            a.rows_ptr(), mptr<float>(y), a.stream()))
        raise_lib();
    return y;
}

// need_x, need_table -> (dL_dx [N,3], dL_dtable [rows,F]), None where not asked for; grad_out [N, L*F]
py::tuple hashgrid_rows_backward(In x, In table, const std::vector<int64_t>& resolutions, int64_t log2_T, const std::optional<at::Tensor>& n_rows,
                                 In grad_out, bool need_x, bool need_table) {
    const HashGridArgs a = hashgrid_args(x, table, resolutions, log2_T, n_rows);
    c10::DeviceGuard guard(a.dev);
    check_grad_out(a, grad_out, a.L * a.F, "L * F");
    const at::Tensor go = f32(grad_out, "grad_out");
    at::Tensor dx = grad_if(need_x, {a.N, 3}, a.dev), dt = grad_if(need_table, {a.rows, a.F}, a.dev);
    if (g_abi.hashgrid_rows_backward((int)a.N, (int)a.L, (int)a.F, a.log2_T, a.res.data(), mptr<const float>(a.x),
                                     reinterpret_cast<const float*>(a.table.data_ptr()), a.rows_ptr(), mptr<const float>(go), out_ptr(dx), out_ptr(dt),
                                     a.stream()))
        raise_lib();
    return py::make_tuple(or_none(dx), or_none(dt));
}

// -- packed_row_views / sh_rows: the view direction of packed rows as spherical harmonics (dmesh_renderer_amd_sh.h).
// -> view i32 [rows]: the view of the slot that owns each packed row, -1 where no slot does
at::Tensor packed_row_views(In row, int64_t rows) {
    built(g_abi.packed_row_views, "dmr_packed_row_views");
    const c10::Device dev = hip_device_of(row);
    if (row.dim() != 4) err("row must have dimensions (B, K, H, W)");
    if (rows < 0 || rows >= ((int64_t)1 << 31)) err("packed_row_views: rows must be in 0..2^31 - 1");
    const int64_t B = row.size(0), K = row.size(1), H = row.size(2), W = row.size(3);
    if (B * K * H * W >= ((int64_t)1 << 31)) err("packed_row_views: B K H W must be below 2^31");
    const at::Tensor r = i32(row, "row");
    c10::DeviceGuard guard(dev);
    if (B * H * W == 0) return at::full({rows}, -1, at::TensorOptions().dtype(at::kInt).device(dev));  // (the C call enqueues nothing)
    at::Tensor view = at::empty({rows}, at::TensorOptions().dtype(at::kInt).device(dev));
    if (g_abi.packed_row_views((int)B, (int)K, (int)H, (int)W, (int)rows, mptr<const int32_t>(r), mptr<int32_t>(view), stream_on(dev))) raise_lib();
    return view;
}

struct ShArgs : RowArgs {
    at::Tensor origin, row_view;
    int64_t B = 0, degree = 0;
    const float* origin_ptr() const { return origin.defined() ? reinterpret_cast<const float*>(origin.data_ptr()) : nullptr; }
    const int32_t* view_ptr() const { return row_view.defined() ? reinterpret_cast<const int32_t*>(row_view.data_ptr()) : nullptr; }
};

ShArgs sh_args(In x, int64_t degree, const std::optional<at::Tensor>& origin, const std::optional<at::Tensor>& row_view,
               const std::optional<at::Tensor>& n_rows) {
    ShArgs a;
    rows_begin(a, "sh_rows", g_abi.sh_rows, x, 3, "3");
    a.degree = degree;
    if (degree < 1 || degree > DMR_SH_MAX_DEGREE) err("sh_rows: degree must be in 1..4, got " + std::to_string(degree));
    if (origin) {
        if (origin->dim() != 2 || origin->size(1) != 3) err("origin must have dimensions (views, 3)");
        a.B = origin->size(0);
        if (a.B < 1 || a.B > DMR_SH_MAX_VIEWS) err("sh_rows: 1 to " + std::to_string(DMR_SH_MAX_VIEWS) + " views, got " + std::to_string(a.B));
    }
    if (row_view && !origin) err("sh_rows: row_view without origin");
    if (row_view && (row_view->dim() != 1 || row_view->size(0) != a.N)) err("row_view must have dimensions (rows)");
    check_row_count(a);
    check_n_rows(n_rows);
    on_device_of_x(a, origin, "sh_rows: origin");
    on_device_of_x(a, row_view, "sh_rows: row_view");
    rows_devices_end(a, x, n_rows);
    if (origin) a.origin = f32(*origin, "origin");
    if (row_view) a.row_view = i32(*row_view, "row_view");
    rows_finish(a, n_rows);
    return a;
}

// -> y [N, degree^2]
at::Tensor sh_rows(In x, int64_t degree, const std::optional<at::Tensor>& origin, const std::optional<at::Tensor>& row_view,
                   const std::optional<at::Tensor>& n_rows) {
    const ShArgs a = sh_args(x, degree, origin, row_view, n_rows);
    c10::DeviceGuard guard(a.dev);
    at::Tensor y = at::empty({a.N, a.degree * a.degree}, f32_on(a.dev));
    if (g_abi.sh_rows((int)a.N, (int)a.degree, (int)a.B, mptr<const float>(a.x), a.origin_ptr(), a.N ? a.view_ptr() : nullptr, a.rows_ptr(),
                      mptr<float>(y), a.stream()))
        raise_lib();
    return y;
}

// need_x, need_origin -> (dL_dx [N,3], dL_dorigin [B,3]), None where not asked for; grad_out [N, degree^2]
py::tuple sh_rows_backward(In x, int64_t degree, const std::optional<at::Tensor>& origin, const std::optional<at::Tensor>& row_view,
                           const std::optional<at::Tensor>& n_rows, In grad_out, bool need_x, bool need_origin) {
    const ShArgs a = sh_args(x, degree, origin, row_view, n_rows);
    c10::DeviceGuard guard(a.dev);
    check_grad_out(a, grad_out, a.degree * a.degree, "degree^2");
    if (need_origin && !origin) err("sh_rows_backward: need_origin without origin");
    const at::Tensor go = f32(grad_out, "grad_out");
    at::Tensor dx = grad_if(need_x, {a.N, 3}, a.dev), dorg = grad_if(need_origin, {a.B, 3}, a.dev);
    if (g_abi.sh_rows_backward((int)a.N, (int)a.degree, (int)a.B, mptr<const float>(a.x), a.origin_ptr(), a.N ? a.view_ptr() : nullptr, a.rows_ptr(),
                               mptr<const float>(go), out_ptr(dx), out_ptr(dorg), a.stream()))
        raise_lib();
    return py::make_tuple(or_none(dx), or_none(dorg));
}

// -- envmap_rows: direction rows looked up in a lat-long environment map (dmesh_renderer_amd_envmap.h).  envmap [He,We,C].
struct EnvMapArgs : RowArgs {
    at::Tensor envmap;
    int64_t He = 0, We = 0, C = 0;
};

EnvMapArgs envmap_args(In d, In envmap, const std::optional<at::Tensor>& n_rows) {
    EnvMapArgs a;
    rows_begin(a, "envmap_rows", g_abi.envmap_rows, d, 3, "3");
    if (envmap.dim() != 3) err("envmap must have dimensions (He, We, C)");
    a.He = envmap.size(0); a.We = envmap.size(1); a.C = envmap.size(2);
    if (a.C < 1 || a.C > DMR_ENVMAP_MAX_CHANNELS) err("envmap_rows: C must be in 1..16, got " + std::to_string(a.C));
    if (a.He < 1 || a.We < 1) err("envmap_rows: the map must have at least one texel");
    if (a.He * a.We * ((a.C + 3) / 4) >= ((int64_t)1 << 31)) err("envmap_rows: He * We * ceil(C / 4) must be below 2^31");
    check_row_count(a);
    check_n_rows(n_rows);
    on_device_of_x(a, envmap, "envmap_rows: envmap");
    rows_devices_end(a, d, n_rows);
    a.envmap = f32(envmap, "envmap");
    rows_finish(a, n_rows);
    return a;
}

// -> y [N,C]
at::Tensor envmap_rows(In d, In envmap, const std::optional<at::Tensor>& n_rows) {
    const EnvMapArgs a = envmap_args(d, envmap, n_rows);
    c10::DeviceGuard guard(a.dev);
    at::Tensor y = at::empty({a.N, a.C}, f32_on(a.dev));
    if (g_abi.envmap_rows((int)a.N, (int)a.C, (int)a.He, (int)a.We, mptr<const float>(a.x), mptr<const float>(a.envmap), a.rows_ptr(), mptr<float>(y),
                          a.stream()))
        raise_lib();
    return y;
}

// need_d, need_envmap -> (dL_dd [N,3], dL_denvmap [He,We,C]), None where not asked for; grad_out [N,C]
py::tuple envmap_rows_backward(In d, In envmap, const std::optional<at::Tensor>& n_rows, In grad_out, bool need_d, bool need_envmap) {
    const EnvMapArgs a = envmap_args(d, envmap, n_rows);
    c10::DeviceGuard guard(a.dev);
    check_grad_out(a, grad_out, a.C, "C");
    const at::Tensor go = f32(grad_out, "grad_out");
    at::Tensor dd = grad_if(need_d, {a.N, 3}, a.dev), de = grad_if(need_envmap, {a.He, a.We, a.C}, a.dev);
    if (g_abi.envmap_rows_backward((int)a.N, (int)a.C, (int)a.He, (int)a.We, mptr<const float>(a.x), mptr<const float>(a.envmap), a.rows_ptr(),
                                   mptr<const float>(go), out_ptr(dd), out_ptr(de), a.stream()))
        raise_lib();
    return py::make_tuple(or_none(dd), or_none(de));
}

// -- envmap_pyramid / envmap_lod_rows: a mip pyramid of a lat-long map and direction rows looked up in it at a per-row level of
// detail (dmesh_renderer_amd_envmap_lod.h).  The spec (He, We, L) -> T, the pyramid's rows; `call` starts the messages.
int64_t pyramid_rows(const char* call, int64_t C, int64_t He, int64_t We, int64_t L) {
    const std::string n = std::string(call) + ": ";
    if (C < 1 || C > DMR_ENVMAP_LOD_MAX_CHANNELS) err(n + "C must be in 1..16, got " + std::to_string(C));
    if (L < 1 || L > DMR_ENVMAP_LOD_MAX_LEVELS) err(n + "levels must be in 1..12, got " + std::to_string(L));
    if (He < 1 || We < 1) err(n + "the map must have at least one texel");
    const int64_t mask = ((int64_t)1 << (L - 1)) - 1;
    if ((He & mask) || (We & mask)) err(n + "He and We must be multiples of 2^(levels-1)");
    int64_t T = 0;
    for (int64_t l = 0; l < L; l++) T += (He >> l) * (We >> l);
    if (T * ((C + 3) / 4) >= ((int64_t)1 << 31)) err(n + "T * ceil(C / 4) must be below 2^31");
    return T;
}

// envmap [He,We,C] -> pyramid [T,C]
at::Tensor envmap_pyramid(In envmap, int64_t levels) {
    built(g_abi.envmap_pyramid, "dmr_envmap_pyramid");
    const c10::Device dev = hip_device_of(envmap);
    if (envmap.dim() != 3) err("envmap must have dimensions (He, We, C)");
    const int64_t He = envmap.size(0), We = envmap.size(1), C = envmap.size(2);
    const int64_t T = pyramid_rows("envmap_pyramid", C, He, We, levels);
    const at::Tensor e = f32(envmap, "envmap");
    c10::DeviceGuard guard(dev);
    at::Tensor pyramid = at::empty({T, C}, f32_on(dev));
    if (g_abi.envmap_pyramid((int)C, (int)He, (int)We, (int)levels, mptr<const float>(e), mptr<float>(pyramid), stream_on(dev))) raise_lib();
    return pyramid;
}

// grad_pyramid [T,C] -> dL_denvmap [He,We,C]
at::Tensor envmap_pyramid_backward(In grad_pyramid, int64_t He, int64_t We, int64_t levels) {
    built(g_abi.envmap_pyramid_backward, "dmr_envmap_pyramid_backward");
    const c10::Device dev = hip_device_of(grad_pyramid);
    if (grad_pyramid.dim() != 2) err("grad_pyramid must have dimensions (T, C)");
    const int64_t C = grad_pyramid.size(1);
    if (pyramid_rows("envmap_pyramid_backward", C, He, We, levels) != grad_pyramid.size(0)) err("grad_pyramid must have dimensions (T, C) of the spec");
    const at::Tensor g = f32(grad_pyramid, "grad_pyramid");
    c10::DeviceGuard guard(dev);
    at::Tensor de = at::empty({He, We, C}, f32_on(dev));
    if (g_abi.envmap_pyramid_backward((int)C, (int)He, (int)We, (int)levels, mptr<const float>(g), mptr<float>(de), stream_on(dev))) raise_lib();
    return de;
}

struct EnvLodArgs : RowArgs {
    at::Tensor lod, pyramid;  // lod: a 1-D view, read in place at its own stride
    int64_t He = 0, We = 0, L = 0, C = 0, T = 0, lod_stride = 1;
    const float* lod_ptr() const { return N ? lod.data_ptr<float>() : nullptr; }
};

EnvLodArgs envmap_lod_args(In d, In lod, In pyramid, int64_t He, int64_t We, int64_t levels, const std::optional<at::Tensor>& n_rows) {
    EnvLodArgs a;
    rows_begin(a, "envmap_lod_rows", g_abi.envmap_lod_rows, d, 3, "3");
    if (!(lod.dim() == 1 || (lod.dim() == 2 && lod.size(1) == 1)) || lod.size(0) != a.N) err("lod must have dimensions (rows,) or (rows, 1)");
    if (pyramid.dim() != 2) err("pyramid must have dimensions (T, C)");
    a.He = He; a.We = We; a.L = levels; a.C = pyramid.size(1);
    a.T = pyramid_rows("envmap_lod_rows", a.C, He, We, levels);
    if (pyramid.size(0) != a.T) err("envmap_lod_rows: pyramid must have the " + std::to_string(a.T) + " rows of the spec, got " + std::to_string(pyramid.size(0)));
    check_row_count(a);
    check_n_rows(n_rows);
    on_device_of_x(a, lod, "envmap_lod_rows: lod");
    on_device_of_x(a, pyramid, "envmap_lod_rows: pyramid");
    rows_devices_end(a, d, n_rows);
    if (lod.scalar_type() != at::kFloat) err("expected scalar type Float but found " + dtype_name(lod) + " (lod)");
    a.lod = lod.dim() == 2 ? lod.select(1, 0) : lod;
    if (a.N > 1 && (a.lod.stride(0) < 1 || a.lod.stride(0) > INT32_MAX)) a.lod = a.lod.contiguous();  // (an expanded or flipped view)
    a.lod_stride = a.N > 1 ? a.lod.stride(0) : 1;
    a.pyramid = f32(pyramid, "pyramid");
    rows_finish(a, n_rows);
    return a;
}

// -> y [N,C]
at::Tensor envmap_lod_rows(In d, In lod, In pyramid, int64_t He, int64_t We, int64_t levels, const std::optional<at::Tensor>& n_rows) {
    const EnvLodArgs a = envmap_lod_args(d, lod, pyramid, He, We, levels, n_rows);
    c10::DeviceGuard guard(a.dev);
    at::Tensor y = at::empty({a.N, a.C}, f32_on(a.dev));
    if (g_abi.envmap_lod_rows((int)a.N, (int)a.C, (int)a.He, (int)a.We, (int)a.L, (int)a.lod_stride, mptr<const float>(a.x), a.lod_ptr(),
                              mptr<const float>(a.pyramid), a.rows_ptr(), mptr<float>(y), a.stream()))
        raise_lib();
    return y;
}

// need_d, need_lod, need_pyramid -> (dL_dd [N,3], dL_dlod [N], dL_dpyramid [T,C]), None where not asked for; grad_out [N,C]
py::tuple envmap_lod_rows_backward(In d, In lod, In pyramid, int64_t He, int64_t We, int64_t levels, const std::optional<at::Tensor>& n_rows,
                                   In grad_out, bool need_d, bool need_lod, bool need_pyramid) {
    const EnvLodArgs a = envmap_lod_args(d, lod, pyramid, He, We, levels, n_rows);
    c10::DeviceGuard guard(a.dev);
    check_grad_out(a, grad_out, a.C, "C");
    const at::Tensor go = f32(grad_out, "grad_out");
    at::Tensor dd = grad_if(need_d, {a.N, 3}, a.dev), dl = grad_if(need_lod, {a.N}, a.dev), dp = grad_if(need_pyramid, {a.T, a.C}, a.dev);
    if (g_abi.envmap_lod_rows_backward((int)a.N, (int)a.C, (int)a.He, (int)a.We, (int)a.L, (int)a.lod_stride, mptr<const float>(a.x), a.lod_ptr(),
                                       mptr<const float>(a.pyramid), a.rows_ptr(), mptr<const float>(go), out_ptr(dd), out_ptr(dl), out_ptr(dp),
                                       a.stream()))
        raise_lib();
    return py::make_tuple(or_none(dd), or_none(dl), or_none(dp));
}

py::tuple profile_collect() {
    std::vector<double> ms(DMR_NUM_STAGES, 0.0);
    std::vector<int64_t> cnt(DMR_NUM_STAGES, 0);
    if (g_abi.profile_collect(ms.data(), cnt.data())) raise_lib();
    return py::make_tuple(ms, cnt);
}

// render_tris / render_tets as bound: run with the GIL released (the default call waits for the size read-back); the one place
// the tuple's length is decided -- cut to the reference's seven unless fragments (the last argument) = K > 0.
template <class R, class... A>
auto bind_forward(R (*fn)(A...)) {
    return [fn](A... a) {
        R out;
        {
            py::gil_scoped_release nogil;
            out = fn(a...);
        }
        const py::tuple all = py::cast(out);
        return std::get<sizeof...(A) - 1>(std::forward_as_tuple(a...)) > 0 ? all : py::tuple(all[py::slice(0, 7, 1)]);
    };
}

}  // namespace

PYBIND11_MODULE(_C, m) {
    load_abi();  // import fails loudly when the HIP library is missing or mismatched
    m.doc() = "dmesh_renderer_amd._C: the reference's four-function binding surface (ext.cpp:6-11) over libdmesh_renderer_hip.so";
    const auto rows = py::arg("rows") = std::pair<int, int>(0, 0), alpha = py::arg("alpha") = false;
    const auto flat_out = py::arg("flat_out") = py::none(), camera_grads = py::arg("camera_grads") = false;
    const auto def = [&m](const char* name, auto fn, const auto&... more) {  // the arguments every render_* function starts with
        m.def(name, fn, py::arg("background"), py::arg("verts"), py::arg("faces"), py::arg("verts_color"), py::arg("faces_opacity"),
              py::arg("mv_mats"), py::arg("proj_mats"), py::arg("inv_mv_mats"), py::arg("inv_proj_mats"), py::arg("verts_depth"),
              py::arg("faces_intense"), more...);
    };
    def("render_tris", bind_forward(&render_tris),
        py::arg("image_height"), py::arg("image_width"), rows, py::arg("fill_outside") = true, py::kw_only(), alpha, py::arg("fragments") = 0);
    def("render_tris_backward", &render_tris_backward, py::arg("dL_dout_color"), py::arg("dL_dout_depth"), py::arg("R"), py::arg("pointBuffer"),
        py::arg("faceBuffer"), py::arg("binningBuffer"), py::arg("imageBuffer"), rows, flat_out, py::kw_only(), py::arg("exact_grads") = false,
        camera_grads, alpha, py::arg("fragment_grads") = py::none());
    def("render_tets", bind_forward(&render_tets),
        py::arg("tets"), py::arg("face_tets"), py::arg("tet_faces"), py::arg("image_height"), py::arg("image_width"), py::arg("ray_random_seed"), rows,
        py::kw_only(), alpha, py::arg("fragments") = 0);
    def("render_tets_backward", &render_tets_backward, py::arg("tets"), py::arg("face_tets"), py::arg("tet_faces"), py::arg("grad_color"),
        py::arg("grad_depth"), py::arg("pointBuffer"), py::arg("faceBuffer"), py::arg("binningBuffer"), py::arg("imageBuffer"), rows, flat_out,
        py::kw_only(), py::arg("full_grads") = false, camera_grads, alpha, py::arg("fragment_grads") = py::none());
    m.def("invert_mats", &invert_mats);
    m.def("composite_fragments", &composite_fragments, py::arg("face"), py::arg("bary"), py::arg("faces"), py::arg("faces_opacity"),
          py::arg("vert_attrs"), py::arg("face_scale") = py::none());
    m.def("composite_fragments_backward", &composite_fragments_backward, py::arg("face"), py::arg("bary"), py::arg("faces"),
          py::arg("faces_opacity"), py::arg("vert_attrs"), py::arg("face_scale"), py::arg("grad_image"), py::arg("grad_T"),
          py::arg("need") = std::array<bool, 4>{true, true, true, true});
    m.def("composite_texture", &composite_texture, py::arg("face"), py::arg("bary"), py::arg("uv_faces"), py::arg("faces_opacity"),
          py::arg("vert_uvs"), py::arg("texture"), py::arg("face_scale") = py::none(), py::arg("wrap") = 0);
    m.def("composite_texture_backward", &composite_texture_backward, py::arg("face"), py::arg("bary"), py::arg("uv_faces"),
          py::arg("faces_opacity"), py::arg("vert_uvs"), py::arg("texture"), py::arg("face_scale"), py::arg("wrap"), py::arg("grad_image"),
          py::arg("grad_T"), py::arg("need") = std::array<bool, 5>{true, true, true, true, true});
    m.def("face_visibility", &face_visibility, py::arg("face"), py::arg("faces_opacity"), py::arg("pixel_weight") = py::none(),
          py::arg("coverage") = false);
    m.def("face_visibility_backward", &face_visibility_backward, py::arg("face"), py::arg("faces_opacity"), py::arg("pixel_weight"),
          py::arg("grad_vis"), py::arg("need") = std::array<bool, 2>{true, true});
    m.def("interpolate_fragments", &interpolate_fragments, py::arg("face"), py::arg("bary"), py::arg("faces"), py::arg("vert_attrs"));
    m.def("interpolate_fragments_backward", &interpolate_fragments_backward, py::arg("face"), py::arg("bary"), py::arg("faces"),
          py::arg("vert_attrs"), py::arg("grad_out"), py::arg("need") = std::array<bool, 2>{true, true});
    m.def("composite_values", &composite_values, py::arg("face"), py::arg("faces_opacity"), py::arg("values"), py::arg("face_scale") = py::none());
    m.def("composite_values_backward", &composite_values_backward, py::arg("face"), py::arg("faces_opacity"), py::arg("values"),
          py::arg("face_scale"), py::arg("grad_image"), py::arg("grad_T"), py::arg("need") = std::array<bool, 3>{true, true, true});
    m.def("pack_slots", &pack_slots, py::arg("face"), py::arg("F"), py::arg("capacity"));
    m.def("interpolate_packed", &interpolate_packed, py::arg("face"), py::arg("bary"), py::arg("row"), py::arg("n_used"), py::arg("faces"),
          py::arg("vert_attrs"), py::arg("rows"));
    m.def("interpolate_packed_backward", &interpolate_packed_backward, py::arg("face"), py::arg("bary"), py::arg("row"), py::arg("n_used"),
          py::arg("faces"), py::arg("vert_attrs"), py::arg("grad_out"), py::arg("need") = std::array<bool, 2>{true, true});
    m.def("composite_values_packed", &composite_values_packed, py::arg("face"), py::arg("row"), py::arg("faces_opacity"), py::arg("values"),
          py::arg("face_scale") = py::none());
    m.def("composite_values_packed_backward", &composite_values_packed_backward, py::arg("face"), py::arg("row"), py::arg("n_used"),
          py::arg("faces_opacity"), py::arg("values"), py::arg("face_scale"), py::arg("grad_image"), py::arg("grad_T"),
          py::arg("need") = std::array<bool, 3>{true, true, true});
    m.def("mlp_rows", &mlp_rows, py::arg("x"), py::arg("weights"), py::arg("biases"), py::arg("act"), py::arg("oact"), py::arg("n_rows") = py::none());
    m.def("mlp_rows_backward", &mlp_rows_backward, py::arg("x"), py::arg("weights"), py::arg("biases"), py::arg("act"), py::arg("oact"),
          py::arg("n_rows"), py::arg("grad_out"), py::arg("need_x"), py::arg("need_w"), py::arg("need_b"));
    m.def("hashgrid_rows", &hashgrid_rows, py::arg("x"), py::arg("table"), py::arg("resolutions"), py::arg("log2_T"), py::arg("n_rows") = py::none());
    m.def("hashgrid_rows_backward", &hashgrid_rows_backward, py::arg("x"), py::arg("table"), py::arg("resolutions"), py::arg("log2_T"),
          py::arg("n_rows"), py::arg("grad_out"), py::arg("need_x"), py::arg("need_table"));
    m.def("packed_row_views", &packed_row_views, py::arg("row"), py::arg("rows"));
    m.def("sh_rows", &sh_rows, py::arg("x"), py::arg("degree"), py::arg("origin") = py::none(), py::arg("row_view") = py::none(),
          py::arg("n_rows") = py::none());
    m.def("sh_rows_backward", &sh_rows_backward, py::arg("x"), py::arg("degree"), py::arg("origin"), py::arg("row_view"), py::arg("n_rows"),
          py::arg("grad_out"), py::arg("need_x"), py::arg("need_origin"));
    m.def("envmap_rows", &envmap_rows, py::arg("d"), py::arg("envmap"), py::arg("n_rows") = py::none());
    m.def("envmap_rows_backward", &envmap_rows_backward, py::arg("d"), py::arg("envmap"), py::arg("n_rows"), py::arg("grad_out"), py::arg("need_d"),
          py::arg("need_envmap"));
    m.def("envmap_pyramid", &envmap_pyramid, py::arg("envmap"), py::arg("levels"));
    m.def("envmap_pyramid_backward", &envmap_pyramid_backward, py::arg("grad_pyramid"), py::arg("He"), py::arg("We"), py::arg("levels"));
    m.def("envmap_lod_rows", &envmap_lod_rows, py::arg("d"), py::arg("lod"), py::arg("pyramid"), py::arg("He"), py::arg("We"), py::arg("levels"),
          py::arg("n_rows") = py::none());
    m.def("envmap_lod_rows_backward", &envmap_lod_rows_backward, py::arg("d"), py::arg("lod"), py::arg("pyramid"), py::arg("He"), py::arg("We"),
          py::arg("levels"), py::arg("n_rows"), py::arg("grad_out"), py::arg("need_d"), py::arg("need_lod"), py::arg("need_pyramid"));
    m.def("surface_packed", &surface_packed, py::arg("face"), py::arg("bary"), py::arg("row"), py::arg("n_used"), py::arg("faces"), py::arg("verts"),
          py::arg("origin"), py::arg("rows"));
    m.def("surface_packed_backward", &surface_packed_backward, py::arg("face"), py::arg("bary"), py::arg("row"), py::arg("n_used"), py::arg("faces"),
          py::arg("verts"), py::arg("origin"), py::arg("grad_hit"), py::arg("grad_normal"), py::arg("grad_reflect"),
          py::arg("need") = std::array<bool, 3>{true, true, true});
    m.def("export", &export_item, py::arg("name"), py::arg("call_args"), py::arg("is_tet"), py::arg("num_rendered"), py::arg("buffers"),
          py::arg("H"), py::arg("W"), py::arg("dtype"));
    // asynchronous calls (include/dmesh_renderer_amd.h, "Sizes only the device knows")
    m.def("set_async", [](bool on) { g_async.store(on ? 1 : 0); }, py::arg("on"),
          "Calls never wait for the device: num_rendered is the capacity used; check overflowed() after synchronising.");
    m.def("is_async", []() { return g_async.load() != 0; });
    m.def("redo_count", []() { return (unsigned long long)g_abi.redo_count(); },
          "Default calls that had to enqueue stages twice because a size estimate was too small (process-wide).");
    m.def("overflowed", [](int device, bool reset) { return g_abi.overflowed(device, reset ? 1 : 0) != 0; }, py::arg("device") = -1,
          py::arg("reset") = true, "True if an asynchronous / graph-captured call outgrew its buffers since the last reset.");
    // per-stage HIP-event timing (bench.py's roofline leg)
    m.def("profile_enable", [](uint32_t mask) { g_abi.profile_enable(mask); }, py::arg("mask"));
    m.def("profile_collect", &profile_collect, "-> (ms per stage, launches per stage), accumulated since the last call");
    m.def("stage_name", [](int i) { return std::string(g_abi.stage_name(i)); });
    m.def("last_error", []() { return std::string(g_abi.last_error()); });
    m.def("library_path", []() { return g_abi.path; });
    m.def("build_arch", []() { return std::string(g_abi.build_arch()); });
    m.attr("NUM_STAGES") = (int)DMR_NUM_STAGES;
    m.attr("ABI_VERSION") = (int)DMR_ABI_VERSION;
    m.attr("NUM_CHANNELS") = NUM_CHANNELS;
    m.attr("SUPPORTS_FLAT_OUT") = true;  // render_*_backward(flat_out=...), used by sharding.py
    m.attr("SUPPORTS_TET_FRAGMENT_GRADS") = true;  // render_tets_backward(fragment_grads=...), asked for by TetRenderer(fragment_grads=True)
    // fragments.composite_fused; False: the loaded library predates dmesh_renderer_amd_shade.h
    m.attr("SUPPORTS_FRAGMENT_COMPOSITE") = g_abi.composite_fragments != nullptr;
    // fragments.composite_texture_fused; False: the loaded library predates dmesh_renderer_amd_texture.h
    m.attr("SUPPORTS_FRAGMENT_TEXTURE") = g_abi.composite_texture != nullptr;
    // fragments.face_visibility_fused; False: the loaded library predates dmesh_renderer_amd_visibility.h
    m.attr("SUPPORTS_FRAGMENT_VISIBILITY") = g_abi.face_visibility != nullptr;
    // fragments.interpolate_fused / composite_values_fused; False: the loaded library predates dmesh_renderer_amd_deferred.h
    m.attr("SUPPORTS_FRAGMENT_DEFERRED") = g_abi.interpolate_fragments != nullptr;
    // fragments.pack_slots_fused / interpolate_packed_fused / composite_values_packed_fused; False: the loaded library predates
    // dmesh_renderer_amd_packed.h
    m.attr("SUPPORTS_FRAGMENT_PACKED") = g_abi.pack_slots != nullptr;
    // fragments.mlp_rows_fused; False: the loaded library predates dmesh_renderer_amd_mlp.h
    m.attr("SUPPORTS_FRAGMENT_MLP") = g_abi.mlp_rows != nullptr;
    // fragments.hashgrid_rows_fused; False: the loaded library predates dmesh_renderer_amd_hashgrid.h
    m.attr("SUPPORTS_FRAGMENT_HASHGRID") = g_abi.hashgrid_rows != nullptr;
    // fragments.packed_row_views_fused / sh_rows_fused; False: the loaded library predates dmesh_renderer_amd_sh.h
    m.attr("SUPPORTS_FRAGMENT_SH") = g_abi.sh_rows != nullptr;
    // fragments.envmap_rows_fused; False: the loaded library predates dmesh_renderer_amd_envmap.h
    m.attr("SUPPORTS_FRAGMENT_ENVMAP") = g_abi.envmap_rows != nullptr;
    // fragments.envmap_pyramid_fused / envmap_lod_rows_fused; False: the loaded library predates dmesh_renderer_amd_envmap_lod.h
    m.attr("SUPPORTS_FRAGMENT_ENVMAP_LOD") = g_abi.envmap_lod_rows != nullptr;
    // fragments.surface_packed_fused; False: the loaded library predates dmesh_renderer_amd_surface.h
    m.attr("SUPPORTS_FRAGMENT_SURFACE") = g_abi.surface_packed != nullptr;
    m.attr("STAGE_PROJECT") = (int)DMR_STAGE_PROJECT; m.attr("STAGE_SETUP_FACES") = (int)DMR_STAGE_SETUP_FACES;
    m.attr("STAGE_SCAN") = (int)DMR_STAGE_SCAN; m.attr("STAGE_SCATTER") = (int)DMR_STAGE_SCATTER; m.attr("STAGE_SORT") = (int)DMR_STAGE_SORT;
    m.attr("STAGE_TRI_FORWARD") = (int)DMR_STAGE_TRI_FORWARD; m.attr("STAGE_TRI_BACKWARD") = (int)DMR_STAGE_TRI_BACKWARD;
    m.attr("STAGE_TRI_UNPACK") = (int)DMR_STAGE_TRI_UNPACK; m.attr("STAGE_TET_FIRST") = (int)DMR_STAGE_TET_FIRST;
    m.attr("STAGE_TET_FORWARD") = (int)DMR_STAGE_TET_FORWARD; m.attr("STAGE_TET_BACKWARD") = (int)DMR_STAGE_TET_BACKWARD;
    m.attr("STAGE_TRI_BACKWARD_HITS") = (int)DMR_STAGE_TRI_BACKWARD_HITS;
}
