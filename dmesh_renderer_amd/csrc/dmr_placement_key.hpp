// dmr_placement_key.hpp -- key of the speculative tile-segment placements (dmr_api.hip).  Plain C++, no HIP: the CPU tests
// compile it on its own (tests/test_placement_key_cpu.py).
#pragma once

#include <cstring>

namespace dmr {

// A placement is device memory, so its key starts with the device ordinal; behind it the view configuration the size estimates
// are keyed by (B, W, H, band rows, renderer, floor(log2(B * F))).
struct PlacementKey {
    int device;
    int v[7];
    bool operator<(const PlacementKey& o) const {
        if (device != o.device) return device < o.device;
        return memcmp(v, o.v, sizeof(v)) < 0;
    }
};
inline PlacementKey placement_key(int device, const int* view, int n) {
    PlacementKey k;
    k.device = device;
    for (int i = 0; i < 7; i++) k.v[i] = i < n ? view[i] : 0;
    return k;
}

}  // namespace dmr
