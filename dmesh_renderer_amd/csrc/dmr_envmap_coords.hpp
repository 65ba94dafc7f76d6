// dmr_envmap_coords.hpp -- from a direction row to its place in a lat-long (equirectangular) map: the one function the
// environment unit's memory safety rests on (dmr_envmap.hip; include/dmesh_renderer_amd_envmap.h states the encoding).  Plain C++
// behind DMR_HD, no HIP, in dmr_texture_wrap.hpp's role: the CPU tests compile it on its own with the host compiler
// (tests/test_envmap_cpu.py) and feed it the bits that must not be tried on a GPU.  Whatever the three floats hold, the four
// indices address the map: wrap_pair is the last step before them.
//
// Not contracted to FMA (no fp-contract pragma here: the build's -ffp-contract=off holds), so the host program and the kernels
// run the same arithmetic up to the library's atan2f.
#pragma once

#include <float.h>

#include "dmr_texture_wrap.hpp"

namespace dmr {

constexpr float ENV_MIN_LENGTH = 1e-8f;   // a shorter (or non-finite) |d| is a skipped row
constexpr float ENV_POLE_RHO2 = 1e-12f;   // ux^2 + uy^2 below it: phi = 0, and the row's dL/dd is an exact 0
constexpr float ENV_INV_2PI = 0.15915494309189535f, ENV_INV_PI = 0.3183098861837907f;

struct EnvCoords {
    bool skipped;            // |d| not finite or below ENV_MIN_LENGTH: nothing else below is meaningful but the indices (all 0)
    bool pole;               // rho2 < ENV_POLE_RHO2
    float ux, uy, uz, inv;   // u = d / |d| and 1 / |d|
    float rho2;              // ux^2 + uy^2
    float x, y;              // s We - 0.5, t He - 0.5: texel centres at half-integers
    float fx, fy;            // x - floor(x), y - floor(y), from the unwrapped coordinates
    int ix0, ix1, iy0, iy1;  // columns repeat, rows clamp: always inside [0, We) and [0, He)
};

// He, We >= 1
DMR_HD inline EnvCoords env_coords(float dx, float dy, float dz, int He, int We) {
    EnvCoords c = {true, false, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0, 0, 0, 0};
    const float n = sqrtf(dx * dx + dy * dy + dz * dz);
    if (!(n >= ENV_MIN_LENGTH && n <= FLT_MAX)) return c;  // (NaN: false)
    c.skipped = false;
    c.inv = 1.f / n;
    c.ux = dx * c.inv; c.uy = dy * c.inv; c.uz = dz * c.inv;
    c.rho2 = c.ux * c.ux + c.uy * c.uy;
    c.pole = c.rho2 < ENV_POLE_RHO2;
    // acos(clamp(uz, -1, 1)) as atan2(rho, uz): the same angle, without acos' loss of digits next to the poles (there one
    // rounding of uz is 1e-2 texel of a 1024-row map; this form stays below 1e-4)
    const float theta = atan2f(sqrtf(c.rho2), c.uz);
    const float phi = c.pole ? 0.f : atan2f(c.uy, c.ux);
    const float s = phi * ENV_INV_2PI + 0.5f, t = theta * ENV_INV_PI;
    c.x = s * (float)We - 0.5f;
    c.y = t * (float)He - 0.5f;
    const float x0 = floorf(c.x), y0 = floorf(c.y);
    c.fx = c.x - x0; c.fy = c.y - y0;
    wrap_pair(x0, We, 1, c.ix0, c.ix1);
    wrap_pair(y0, He, 0, c.iy0, c.iy1);
    return c;
}

}  // namespace dmr
