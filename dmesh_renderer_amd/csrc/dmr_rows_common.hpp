// dmr_rows_common.hpp -- what the units over packed [N,C] rows (dmr_mlp.hip, dmr_hashgrid.hip, dmr_sh.hip) share, each fact once,
// on top of dmr_shade_common.hpp:
//   device: the n_rows rule (rows_used), a wave's read-back of its own LDS writes (rows_wave_sync) and the contiguous run of row
//           tiles a backward workgroup takes (rows_tile_run);
//   host:   the grid over row tiles (rows_grid), the ladders from a run-time value to a template argument (with_one_of) and from
//           two wanted outputs to two bools (with_wanted), what a *_rows_backward call does between the checks of its pair and its
//           launch (rows_backward_prologue), and the fill of an output with one word (rows_fill_on: defined once, in
//           dmr_rows_common.hip -- a kernel in this header would be compiled into every includer, launched or not).
// The kernels' walks, the parameter blocks and each unit's own checks stay the unit's own text.
#pragma once

#include "dmr_shade_common.hpp"

namespace dmr {

// n 4-byte words at `a` <- value on the stream, by at most 4096 workgroups of 256: a kernel, not a memset node
void rows_fill_on(hipStream_t st, void* a, int64_t n, uint32_t value);

namespace {

// THE n_rows rule (every unit's header states it): rows r >= min(max(n_rows[0], 0), N) are not read.  P: the unit's parameter block.
template <class P>
__device__ __forceinline__ int rows_used(const P& p) {
    if (!p.n_rows) return p.N;
    const int u = p.n_rows[0];
    return u < 0 ? 0 : (u > p.N ? p.N : u);
}
// a wave reads back what its lanes wrote to LDS (no workgroup barrier: the staging areas are per wave)
__device__ __forceinline__ void rows_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}
// the tiles [t0, t1) a workgroup of a backward launch takes: neighbouring rows stay in one workgroup's table
struct RowsTileRun { int t0, t1; };
__device__ __forceinline__ RowsTileRun rows_tile_run(int tiles) {
    const int per = (tiles + (int)gridDim.x - 1) / (int)gridDim.x;
    const int t0 = (int)blockIdx.x * per;
    return {t0, t0 + per < tiles ? t0 + per : tiles};
}

// ---- Host side.  N rows in tiles of `threads` -> the tiles and the workgroups that stride over them
struct RowsGrid { int tiles, groups; };
inline RowsGrid rows_grid(int N, int threads, int max_groups) {
    const int tiles = (int)(((int64_t)N + threads - 1) / threads);
    return {tiles, tiles < max_groups ? tiles : max_groups};
}
// f(std::integral_constant<int, V>) for the V of the list that v equals; the last V takes every other v (the checks refused those)
template <int V, int... Rest, class Fn>
void with_one_of(int v, Fn&& f) {
    if constexpr (sizeof...(Rest) == 0) f(std::integral_constant<int, V>());
    else if (v == V) f(std::integral_constant<int, V>());
    else with_one_of<Rest...>(v, f);
}
// f(first wanted, second wanted) as bool constants for two outputs of which at least one is wanted: f(false, false) is never compiled
template <class Fn>
void with_wanted(bool first, bool second, Fn&& f) {
    if (first && second) f(std::true_type(), std::true_type());
    else if (first) f(std::true_type(), std::false_type());
    else f(std::false_type(), std::true_type());
}
// After the checks both calls of a pair share: grad_out, the unit's own checks (own: the message of the first that failed, or
// null), then dL_dx is dropped where there is no row.  others: one of the unit's further gradients is wanted.
// -> SHADE_LAUNCH, SHADE_DONE (nothing is wanted) or SHADE_FAILED with the error set.
inline int rows_backward_prologue(const char* name, int N, const float* grad_out, const char* own, float*& dL_dx, bool others) {
    if (N > 0 && !grad_out) return api_fail((std::string(name) + ": null grad_out").c_str());
    if (own) return api_fail((std::string(name) + ": " + own).c_str());
    if (N == 0) dL_dx = nullptr;  // (no row to write)
    return (dL_dx || others) ? SHADE_LAUNCH : SHADE_DONE;
}

}  // namespace
}  // namespace dmr
