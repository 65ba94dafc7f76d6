// dmr_envmap_lod_coords.hpp -- from a direction row and a level of detail to its places in a mip pyramid of a lat-long map: the
// functions the pyramid unit's memory safety rests on (dmr_envmap_lod.hip; include/dmesh_renderer_amd_envmap_lod.h states the
// layout and the encoding).  dmr_envmap_coords.hpp's env_coords cut in two -- the angles of a row, formed once, and the place in
// a map of a given size, formed per level -- plus the level choice and a level's offset.  Plain C++ behind DMR_HD, no HIP, in
// dmr_envmap_coords.hpp's role: the CPU tests compile it on its own with the host compiler (tests/test_envmap_lod_cpu.py) and
// feed it the bits that must not be tried on a GPU.  Whatever the floats hold, the indices address their level and the levels
// lie in [0, L-1]: wrap_pair and the clamp of the two levels are the last steps before them.
//
// env_place(env_angles(d).s, .t, He, We) runs env_coords(d, He, We)'s arithmetic operation by operation (not contracted to FMA:
// the build's -ffp-contract=off holds), so level 0 sits where dmr_envmap.hip puts it, bit for bit.
#pragma once

#include <stdint.h>

#include "dmr_envmap_coords.hpp"

namespace dmr {

constexpr int ENV_LOD_MAX_LEVELS = 12;

struct EnvAngles {
    bool skipped;           // |d| not finite or below ENV_MIN_LENGTH: nothing else below is meaningful (all 0)
    bool pole;              // rho2 < ENV_POLE_RHO2
    float ux, uy, uz, inv;  // u = d / |d| and 1 / |d|
    float rho2;             // ux^2 + uy^2
    float s, t;             // phi / (2 pi) + 0.5, theta / pi: the place on the sphere, whatever the map's size
};

DMR_HD inline EnvAngles env_angles(float dx, float dy, float dz) {
    EnvAngles a = {true, false, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const float n = sqrtf(dx * dx + dy * dy + dz * dz);
    if (!(n >= ENV_MIN_LENGTH && n <= FLT_MAX)) return a;  // (NaN: false)
    a.skipped = false;
    a.inv = 1.f / n;
    a.ux = dx * a.inv; a.uy = dy * a.inv; a.uz = dz * a.inv;
    a.rho2 = a.ux * a.ux + a.uy * a.uy;
    a.pole = a.rho2 < ENV_POLE_RHO2;
    const float theta = atan2f(sqrtf(a.rho2), a.uz);
    const float phi = a.pole ? 0.f : atan2f(a.uy, a.ux);
    a.s = phi * ENV_INV_2PI + 0.5f; a.t = theta * ENV_INV_PI;
    return a;
}

struct EnvPlace {
    float x, y;              // s We - 0.5, t He - 0.5: texel centres at half-integers
    float fx, fy;            // x - floor(x), y - floor(y), from the unwrapped coordinates
    int ix0, ix1, iy0, iy1;  // columns repeat, rows clamp: always inside [0, We) and [0, He)
};

// He, We >= 1: the size of the level
DMR_HD inline EnvPlace env_place(float s, float t, int He, int We) {
    EnvPlace c = {0.f, 0.f, 0.f, 0.f, 0, 0, 0, 0};
    c.x = s * (float)We - 0.5f;
    c.y = t * (float)He - 0.5f;
    const float x0 = floorf(c.x), y0 = floorf(c.y);
    c.fx = c.x - x0; c.fy = c.y - y0;
    wrap_pair(x0, We, 1, c.ix0, c.ix1);
    wrap_pair(y0, He, 0, c.iy0, c.iy1);
    return c;
}

struct EnvLodLevels {
    int l0, l1;   // the two adjacent levels: always inside [0, L-1]; l1 = l0 + 1 unless L == 1
    float f;      // the weight of l1, in [0, 1]; 1 - f is l0's
    bool inside;  // 0 < lod < L-1: where dL/dlod is not an exact 0
};

// L >= 1.  lam = lod clamped into [0, L-1] (a NaN becomes 0), l0 = min(floor(lam), L-2), f = lam - l0; L == 1: l0 = l1 = 0, f = 0
DMR_HD inline EnvLodLevels env_lod_levels(float lod, int L) {
    const int last = L > 1 ? L - 1 : 0;
    const float top = (float)last;
    const float lam = lod >= 0.f ? (lod <= top ? lod : top) : 0.f;  // (NaN: both comparisons false)
    EnvLodLevels v;
    v.inside = lod > 0.f && lod < top;
    int l0 = (int)lam;  // lam in [0, 11]: the floor
    l0 = l0 < last - 1 ? l0 : last - 1;
    l0 = l0 > 0 ? l0 : 0;
    v.f = last > 0 ? lam - (float)l0 : 0.f;
    const int l1 = l0 + 1;
    v.l0 = l0 < last ? l0 : last;
    v.l1 = l1 < last ? l1 : last;
    return v;
}

// off_l = sum_{j<l} (He >> j) (We >> j), in texels, for He and We multiples of 2^(L-1) and 0 <= l < L: every level then holds
// exactly a quarter of the one below, and the sum is (4 / 3) (He We - He We / 4^l), the division by 3 exact
DMR_HD inline uint32_t env_lod_offset(int He, int We, int l) {
    const uint32_t hw = (uint32_t)He * (uint32_t)We;
    return (hw - (hw >> (2 * l))) / 3u * 4u;
}

}  // namespace dmr
