// dmr_texture_wrap.hpp -- the index wrap of the texture unit (dmr_texture.hip): the one function the unit's memory safety
// rests on.  Plain C++ behind DMR_HD, no HIP: the CPU tests compile it on its own with the host compiler
// (tests/test_texture_wrap_cpu.py) and feed it the bits that must not be tried on a GPU.
#pragma once

#include <math.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define DMR_HD __host__ __device__
#else
#include <algorithm>
#define DMR_HD
#endif

namespace dmr {

// wrap(x0, n), wrap(x0 + 1, n) of an integer-valued float x0 (or anything else a float can hold): both in [0, n-1].
// wrap: 0 clamp, 1 repeat.  n >= 1.
DMR_HD inline void wrap_pair(float x0, int n, int wrap, int& i0, int& i1) {
#if defined(__clang__)
#pragma clang fp contract(fast)  // (as the unit that calls it: nothing here decides an index another kernel depends on)
#endif
#if !defined(__HIPCC__)
    using std::max;
    using std::min;
#endif
    const float nf = (float)n;
    if (wrap) x0 = x0 - floorf(x0 / nf) * nf;  // remainder, in float: exact while |x0| < 2^24
    x0 = x0 >= -1.f ? x0 : -1.f;               // (false for a NaN too)
    x0 = x0 <= nf ? x0 : nf;
    int i = (int)x0;                           // in [-1, n] (saturated where float(n) rounded up to 2^31)
    if (wrap) {
        if (i < 0) i += n;
        if (i >= n) i -= n;
        i0 = min(max(i, 0), n - 1);
        i1 = i0 + 1 >= n ? 0 : i0 + 1;
    } else {
        i0 = min(max(i, 0), n - 1);
        i1 = max(min(i, n - 2) + 1, 0);        // min(max(i + 1, 0), n - 1) without the overflow of i + 1
    }
}

}  // namespace dmr
