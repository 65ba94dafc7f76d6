"""wrap_pair (csrc/dmr_texture_wrap.hpp) is what the texture unit's memory safety rests on: whatever bits its float holds,
both indices it returns address the texture.  The header is plain C++; this compiles it with the host compiler (the pattern
of tests/test_placement_key_cpu.py) and feeds it, on the CPU, the values that must not be tried on a GPU.

For both wraps, n in {1, 2, 3, 7, 13, 48, 1024, 4096, 2^24}:
  in range   0 <= i0, i1 <= n - 1 for every integer x0 in [-3n - 2, 3n + 2] (n <= 4096; a stride and both ends at 2^24), for
             +-2^k, +-(2^k - 1), +-(2^k + 1) (k <= 24), for k n - 1, k n, k n + n - 1 (|k| up to 2^24 / n), and for the hostile
             values: NaNs of both signs (quiet and signalling bit patterns), +-inf, +-1e30, +-2^31, +-0, the smallest denormal,
             -0.5;
  the model  whenever x0 is integer-valued with |x0| < 2^24: clamp gives clamp(x0, 0, n-1), clamp(x0+1, 0, n-1), repeat gives
             x0 mod n, (x0+1) mod n, the right-hand sides in 64-bit integers (fragments._wrap_index).

n stays <= 2^24 here: the kernel's remark on float(n) rounding up to 2^31 relies on the device's saturating float-to-int
conversion, which the host compiler does not promise (there the conversion of an out-of-range float is undefined).
"""
import os
import shutil
import subprocess
import tempfile

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dmesh_renderer_amd", "csrc")

PROGRAM = r"""
#include <cassert>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <atomic>
#include <limits>
#include <thread>
#include <vector>
#include "dmr_texture_wrap.hpp"

static thread_local long long g_calls = 0, g_modelled = 0;  // (a thread's own; summed when it ends)
static std::atomic<long long> g_all_calls{0}, g_all_modelled{0};

static float from_bits(uint32_t b) { float f; memcpy(&f, &b, sizeof f); return f; }
static int64_t clamp64(int64_t x, int64_t lo, int64_t hi) { return x < lo ? lo : (x > hi ? hi : x); }
static int64_t mod64(int64_t x, int64_t n) { const int64_t r = x % n; return r < 0 ? r + n : r; }

static void check(float x0, int n) {
    for (int wrap = 0; wrap < 2; wrap++) {
        int i0 = -12345, i1 = -12345;
        dmr::wrap_pair(x0, n, wrap, i0, i1);
        g_calls++;
        if (!(i0 >= 0 && i0 <= n - 1 && i1 >= 0 && i1 <= n - 1)) {
            printf("out of range: x0 %a n %d wrap %d -> %d %d\n", x0, n, wrap, i0, i1);
            assert(false);
        }
        if (std::fabs(x0) < 16777216.f && x0 == std::floor(x0)) {  // (false for a NaN)
            const int64_t x = (int64_t)x0;
            const int64_t m0 = wrap ? mod64(x, n) : clamp64(x, 0, n - 1), m1 = wrap ? mod64(x + 1, n) : clamp64(x + 1, 0, n - 1);
            g_modelled++;
            if (i0 != m0 || i1 != m1) {
                printf("model: x0 %a n %d wrap %d -> %d %d, expected %lld %lld\n", x0, n, wrap, i0, i1, (long long)m0, (long long)m1);
                assert(false);
            }
        }
    }
}

int main() {
    const int sizes[9] = {1, 2, 3, 7, 13, 48, 1024, 4096, 1 << 24};
    const float inf = std::numeric_limits<float>::infinity();
    const float hostile[] = {from_bits(0x7fc00000u), from_bits(0xffc00000u), from_bits(0x7fa00000u), from_bits(0xffa00000u),  // q/s NaN
                             from_bits(0x7fffffffu), from_bits(0xff800001u), inf, -inf, 1e30f, -1e30f, 2147483648.f, -2147483648.f,
                             0.f, -0.f, from_bits(0x00000001u), from_bits(0x80000001u), -0.5f};
    for (int n : sizes) {
        const int64_t N = n;
        if (n <= 4096) {
            for (int64_t x = -3 * N - 2; x <= 3 * N + 2; x++) check((float)x, n);
        } else {
            for (int64_t x = -3 * N - 2; x <= 3 * N + 2; x += 4099) check((float)x, n);
            check((float)(-3 * N - 2), n); check((float)(3 * N + 2), n);
            for (int64_t x = -N - 3; x <= -N + 3; x++) check((float)x, n);  // (every integer about -n, 0 and n)
            for (int64_t x = -3; x <= 3; x++) check((float)x, n);
            for (int64_t x = N - 3; x <= N + 3; x++) check((float)x, n);
        }
        for (int k = 0; k <= 24; k++) {
            const float p = (float)((int64_t)1 << k);
            for (float s : {1.f, -1.f}) { check(s * p, n); check(s * (p - 1.f), n); check(s * (p + 1.f), n); }
        }
        // (the long loop: 2^25 / n values of k, split over a few threads)
        const int64_t kmax = ((int64_t)1 << 24) / N, threads = 8, step = (2 * kmax + threads) / threads;
        std::vector<std::thread> pool;
        for (int64_t lo = -kmax; lo <= kmax; lo += step)
            pool.emplace_back([=] {
                for (int64_t k = lo; k < lo + step && k <= kmax; k++) { check((float)(k * N - 1), n); check((float)(k * N), n); check((float)(k * N + N - 1), n); }
                g_all_calls += g_calls; g_all_modelled += g_modelled;
            });
        for (auto& t : pool) t.join();
        for (float h : hostile) check(h, n);
    }
    const long long calls = g_all_calls + g_calls, modelled = g_all_modelled + g_modelled;
    printf("%lld calls, %lld against the integer model\n", calls, modelled);
    assert(modelled > calls / 2);
    return 0;
}
"""


def test_wrap_pair_stays_in_range_and_matches_the_integer_model():
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "wrap.cpp"), os.path.join(tmp, "wrap")
        with open(src, "w") as f:
            f.write(PROGRAM)
        subprocess.run([cxx, "-std=c++17", "-O0", "-UNDEBUG", "-pthread", "-I", CSRC, src, "-o", exe], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
        print("\n" + out.strip())


def test_texture_unit_uses_that_wrap():
    """... and the kernels take their indices from that header's function, not from a copy of their own."""
    unit = open(os.path.join(CSRC, "dmr_texture.hip")).read()
    assert '#include "dmr_texture_wrap.hpp"' in unit
    assert unit.count("wrap_pair(x0, p.Wt, p.wrap, ix0, ix1)") == 1 and unit.count("wrap_pair(y0, p.Ht, p.wrap, iy0, iy1)") == 1
    assert "void wrap_pair(" not in unit
