"""The speculative placements (dmr_api.hip) are device memory: their key must tell devices apart, or a process that renders
one view configuration on two devices would hand one device's arrays to the other.  csrc/dmr_placement_key.hpp is plain
C++; this compiles it with the host compiler and checks the ordering std::map relies on."""
import os
import shutil
import subprocess
import tempfile

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dmesh_renderer_amd", "csrc")

PROGRAM = r"""
#include <cassert>
#include <map>
#include "dmr_placement_key.hpp"
int main() {
    const int view[7] = {1, 1920, 1080, 0, 68, 0, 18};
    const int other[7] = {1, 1920, 1080, 0, 34, 0, 18};
    const dmr::PlacementKey a = dmr::placement_key(0, view, 7), b = dmr::placement_key(1, view, 7), c = dmr::placement_key(0, other, 7);
    assert((a < b) != (b < a));                        // same view configuration, two devices: two keys
    assert((a < c) != (c < a));                        // same device, two bands: two keys
    assert(!(a < dmr::placement_key(0, view, 7)) && !(dmr::placement_key(0, view, 7) < a));
    std::map<dmr::PlacementKey, int> m;
    m[a] = 1; m[b] = 2; m[c] = 3; m[dmr::placement_key(0, view, 7)] = 4;
    assert(m.size() == 3 && m[a] == 4 && m[b] == 2 && m[c] == 3);
    return 0;
}
"""


def test_placement_key_separates_devices():
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "key.cpp"), os.path.join(tmp, "key")
        with open(src, "w") as f:
            f.write(PROGRAM)
        subprocess.run([cxx, "-std=c++17", "-O0", "-UNDEBUG", "-I", CSRC, src, "-o", exe], check=True)
        subprocess.run([exe], check=True)


def test_library_keys_its_placements_by_device():
    """... and the library uses that key (and no other) for its placement map."""
    api = open(os.path.join(CSRC, "dmr_api.hip")).read()
    assert "std::map<dmr::PlacementKey, Placement> g_placement" in api
    assert "dmr::placement_key(current_device()" in api
