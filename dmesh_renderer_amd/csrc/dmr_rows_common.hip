// dmr_rows_common.hip -- the one definition of what dmr_rows_common.hpp declares with external linkage, the row units' fill of an
// output with one word: dL_dtable and dL_dorigin before the backward adds into them (0), view_out before the walk writes it (-1).
#include "dmr_rows_common.hpp"

namespace dmr {
namespace {
__global__ void __launch_bounds__(256) k_rows_fill(uint32_t* __restrict__ a, int64_t n, uint32_t value) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) a[i] = value;
}
}  // namespace

void rows_fill_on(hipStream_t st, void* a, int64_t n, uint32_t value) {
    const int64_t blocks = (n + 255) / 256;
    k_rows_fill<<<dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, st>>>(static_cast<uint32_t*>(a), n, value);
}

}  // namespace dmr
