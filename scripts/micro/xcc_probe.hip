// Probe: which XCD does workgroup b of a 1-D grid run on?  Every workgroup stores HW_REG_XCC_ID; the host checks that the id
// is a function of blockIdx.x % 8 (blocks b and b + 8 share an XCD) and that the 8 residues get 8 different XCDs.
// The placed tile order (dmesh_renderer_amd/csrc/dmr_tile_order.hpp) rests on this observed behaviour for SPEED only.
// Grid sizes 8 160 and 8 161: C4's tiles, and the forward's grid with its one size workgroup in front.
// hipcc --offload-arch=gfx950 -O3 -o xcc_probe xcc_probe.hip && ./xcc_probe
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>
#define CHECK(e) do { hipError_t r_ = (e); if (r_ != hipSuccess) { printf("%s: %s\n", #e, hipGetErrorString(r_)); return 2; } } while (0)

__global__ void __launch_bounds__(256) k_probe(unsigned* out, float* sink, int spin) {
    unsigned id;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(id));
    // some work, so that the grid does not drain faster than it is dispatched (as a compositing kernel's tiles do not)
    float a = (float)threadIdx.x;
    for (int i = 0; i < spin; i++) a = a * 1.0001f + 0.5f;
    if (a == -1.0f) sink[0] = a;
    if (threadIdx.x == 0) out[blockIdx.x] = id & 0xfu;
}

int main() {
    const int grids[2] = {8160, 8161};
    unsigned* out; float* sink;
    CHECK(hipMalloc(&out, 8161 * sizeof(unsigned)));
    CHECK(hipMalloc(&sink, sizeof(float)));
    int bad_total = 0;
    for (int spin : {0, 20000}) {
        for (int n : grids) {
            for (int rep = 0; rep < 3; rep++) {
                CHECK(hipMemset(out, 0xff, 8161 * sizeof(unsigned)));
                k_probe<<<n, 256>>>(out, sink, spin);
                CHECK(hipDeviceSynchronize());
                std::vector<unsigned> h(n);
                CHECK(hipMemcpy(h.data(), out, n * sizeof(unsigned), hipMemcpyDeviceToHost));
                int bad = 0; unsigned seen = 0;
                for (int b = 0; b < n; b++) bad += h[b] != h[b % 8];
                for (int b = 0; b < 8 && b < n; b++) seen |= 1u << h[b];
                printf("grid %d spin %d rep %d: xcc of blocks 0..7 =", n, spin, rep);
                for (int b = 0; b < 8; b++) printf(" %u", h[b]);
                printf("  blocks whose xcc differs from that of block (b %% 8): %d  distinct xccs: %d\n", bad, __builtin_popcount(seen));
                bad_total += bad + (__builtin_popcount(seen) != 8);
            }
        }
    }
    printf(bad_total ? "FAIL: the XCD is not a function of blockIdx.x %% 8\n" : "ok: blocks b and b + 8 share an XCD in every launch\n");
    return bad_total ? 1 : 0;
}
