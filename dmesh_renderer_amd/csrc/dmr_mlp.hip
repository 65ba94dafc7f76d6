// dmr_mlp.hip -- a small MLP over packed, channel-last rows (include/dmesh_renderer_amd_mlp.h): the neural shader between
// dmr_packed.hip's two ends, one forward and one backward kernel.  The model is fragments.mlp_rows:
//     n_hidden = 1    y = oact(W_out act(W_in x + b_in) + b_out)
//     n_hidden = 2    y = oact(W_out act(W_mid act(W_in x + b_in) + b_mid) + b_out)
// A LANE OWNS A ROW.  A layer's outputs live in the lane's registers (the loops over Hd are unrolled: the kernels are templated
// on Hd and on the number of hidden layers), the weights are wave-uniform and come from LDS with same-address (broadcast)
// reads: the workgroup copies them there once, in the orientation each loop reads contiguously (MlpLayout), and then strides
// over its row tiles.  Hidden activations never reach memory; the backward recomputes them from x.
//
// Rows r >= min(max(n_rows[0], 0), N) are not read: y and dL_dx get exact zeros there, and their lanes stage zeros into the
// weight-gradient sums.  Offsets into the [N,C] buffers are int64_t.
#include "dmr_rows_common.hpp"
#include "../../include/dmesh_renderer_amd_mlp.h"

namespace dmr {
namespace {

#pragma clang fp contract(fast)

constexpr int MLP_MAX_CIN = 64, MLP_OUT = 16;  // the rows of the W_in image, the padded width of the output layer
constexpr int MLP_FWD_THREADS = 256, MLP_FWD_MAX_GROUPS = 1024, MLP_BWD_MAX_GROUPS = DMR_MLP_MAX_GROUPS;
// the backward's workgroup: its waves' staging areas, the weights and the table must fit the CU's 160 KiB of LDS
constexpr int mlp_bwd_threads(int hd, int nh) { return hd == 64 && nh == 2 ? 128 : 256; }

struct MlpParams {
    int N, Cin, Cout, act, oact;
    int ovec;  // rows of y / grad_out may be accessed as float4 (Cout % 4 == 0, 16-byte aligned base)
    const float* __restrict__ x;       // [N,Cin]
    const float* __restrict__ w_in;    // [Hd,Cin]
    const float* __restrict__ b_in;    // [Hd] or null
    const float* __restrict__ w_mid;   // [Hd,Hd] (two hidden layers)
    const float* __restrict__ b_mid;   // [Hd] or null
    const float* __restrict__ w_out;   // [Cout,Hd]
    const float* __restrict__ b_out;   // [Cout] or null
    const int32_t* __restrict__ n_rows;  // [1] or null
};

// The weights in LDS, and (same offsets) the backward's table of weight-gradient sums and a workgroup's slice of `scratch`:
//   W1  [c][j]   = W_in[j][c], MLP_MAX_CIN rows of which Cin are used (zeros in the rest)      B1  [j] = b_in
//   W2  [j2][i]  = W_mid[j2][i] (two hidden layers)                                            B2  [j2] = b_mid
//   W3  [j][o]   = W_out[o][j], MLP_OUT columns of which Cout are used (zeros in the rest)      B3  [o] = b_out
// Every loop over Hd (or over the outputs) reads one row of an image: consecutive floats, the same address in every lane.
template <int HD, int NH>
struct MlpLayout {
    static constexpr int W1 = 0, B1 = W1 + MLP_MAX_CIN * HD, W2 = B1 + HD, B2 = W2 + (NH == 2 ? HD * HD : 0), W3 = B2 + (NH == 2 ? HD : 0),
                         B3 = W3 + MLP_OUT * HD, TOTAL = B3 + MLP_OUT;
    static_assert(TOTAL == DMR_MLP_TABLE_FLOATS(HD, NH), "the header states the table's size");
};

template <int HD, int NH, int THREADS>
__device__ __forceinline__ void mlp_load_weights(const MlpParams& p, float* __restrict__ w) {
    using L = MlpLayout<HD, NH>;
    for (int e = threadIdx.x; e < L::TOTAL; e += THREADS) {
        float v = 0.f;
        if (e < L::B1) { const int c = e / HD, j = e % HD; if (c < p.Cin) v = p.w_in[j * p.Cin + c]; }
        else if (e < L::W2) { if (p.b_in) v = p.b_in[e - L::B1]; }
        else if (e < L::B2) v = p.w_mid[e - L::W2];
        else if (e < L::W3) { if (p.b_mid) v = p.b_mid[e - L::B2]; }
        else if (e < L::B3) { const int j = (e - L::W3) / MLP_OUT, o = (e - L::W3) % MLP_OUT; if (o < p.Cout) v = p.w_out[o * HD + j]; }
        else { const int o = e - L::B3; if (o < p.Cout && p.b_out) v = p.b_out[o]; }
        w[e] = v;
    }
}

__device__ __forceinline__ float mlp_act(float z, int act) { return act == DMR_MLP_TANH ? tanhf(z) : (z > 0.f ? z : 0.f); }
// the activation's derivative from its VALUE (relu: a > 0 exactly where z > 0, so 0 at z = 0)
__device__ __forceinline__ float mlp_dact(float a, int act) { return act == DMR_MLP_TANH ? 1.f - a * a : (a > 0.f ? 1.f : 0.f); }

// Between the steps of a fully unrolled loop over Hd whose every step reads its own weights: without it the scheduler hoists
// all Hd steps' LDS reads to the front and the kernel spills (HD = 64: 1024 registers of weights).
__device__ __forceinline__ void mlp_keep_order() { __builtin_amdgcn_sched_barrier(0); }

// h += W_in x, c ascending in both forms (so the float4 and the scalar row loads give the same bits)
template <int HD, bool VEC>
__device__ __forceinline__ void mlp_layer_in(const float* __restrict__ w1, const float* __restrict__ xr, int Cin, float (&h)[HD]) {
    if constexpr (VEC) {
        for (int c = 0; c < Cin; c += 4) {
            const float4 t = *reinterpret_cast<const float4*>(xr + c);
            const float xs[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const float* __restrict__ wr = w1 + (c + q) * HD;
#pragma unroll
                for (int j = 0; j < HD; j++) h[j] += wr[j] * xs[q];
                mlp_keep_order();
            }
        }
    } else {
        for (int c = 0; c < Cin; c++) {
            const float xc = xr[c];
            const float* __restrict__ wr = w1 + c * HD;
#pragma unroll
            for (int j = 0; j < HD; j++) h[j] += wr[j] * xc;
        }
    }
}

// out (preset to b_out) += W_out a, over the MLP_OUT padded outputs, or the first four when Cout <= 4 (uniform)
template <int HD>
__device__ __forceinline__ void mlp_out_add(const float* __restrict__ wo, float a, bool narrow, float (&out)[MLP_OUT]) {
    if (narrow) {
#pragma unroll
        for (int o = 0; o < 4; o++) out[o] += wo[o] * a;
    } else {
#pragma unroll
        for (int o = 0; o < MLP_OUT; o++) out[o] += wo[o] * a;
    }
}

// From the first hidden layer's activations a1 to the pre-activation outputs `out` (preset to b_out).  Two hidden layers: the
// second layer's units one after the other (a rolled loop: each is a dot product of a1 with one row of W_mid), each unit's
// activation straight into the output sums -- and, STAGE, into the lane's row of `second` for the backward.
template <int HD, int NH, bool STAGE>
__device__ __forceinline__ void mlp_tail(const float* __restrict__ w, const float (&a1)[HD], int act, bool narrow, float (&out)[MLP_OUT],
                                         float* __restrict__ second) {
    using L = MlpLayout<HD, NH>;
    if constexpr (NH == 2) {
#pragma unroll 2
        for (int j2 = 0; j2 < HD; j2++) {
            const float* __restrict__ wr = w + L::W2 + j2 * HD;
            float z0 = w[L::B2 + j2], z1 = 0.f;
#pragma unroll
            for (int i = 0; i < HD; i += 2) { z0 += wr[i] * a1[i]; z1 += wr[i + 1] * a1[i + 1]; }
            const float a2 = mlp_act(z0 + z1, act);
            if constexpr (STAGE) second[j2] = a2;
            mlp_out_add<HD>(w + L::W3 + j2 * MLP_OUT, a2, narrow, out);
        }
    } else {
        if (narrow) {
#pragma unroll
            for (int j = 0; j < HD; j++) {
                mlp_out_add<HD>(w + L::W3 + j * MLP_OUT, a1[j], true, out);
                if (j % 8 == 7) mlp_keep_order();
            }
        } else {
#pragma unroll
            for (int j = 0; j < HD; j++) {
                mlp_out_add<HD>(w + L::W3 + j * MLP_OUT, a1[j], false, out);
                if (j % 2 == 1) mlp_keep_order();
            }
        }
    }
}

// ---------------------------------------------------------------------------
// forward.  A workgroup strides over tiles of 256 rows; no barrier after the weights are in.
// ---------------------------------------------------------------------------
template <int HD, int NH, bool VEC>
__global__ void __launch_bounds__(MLP_FWD_THREADS, 2)
k_mlp_rows(MlpParams p, int tiles, float* __restrict__ y) {
    using L = MlpLayout<HD, NH>;
    __shared__ alignas(16) float w[L::TOTAL];
    mlp_load_weights<HD, NH, MLP_FWD_THREADS>(p, w);
    __syncthreads();
    const int n = rows_used(p);
    const bool narrow = p.Cout <= 4;
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t row = (int64_t)tile * MLP_FWD_THREADS + threadIdx.x;
        if (row >= p.N) continue;
        float out[MLP_OUT];
#pragma unroll
        for (int o = 0; o < MLP_OUT; o++) out[o] = 0.f;
        if (row < n) {
            float a1[HD];
#pragma unroll
            for (int j = 0; j < HD; j++) a1[j] = w[L::B1 + j];
            mlp_layer_in<HD, VEC>(w + L::W1, p.x + row * p.Cin, p.Cin, a1);
#pragma unroll
            for (int j = 0; j < HD; j++) a1[j] = mlp_act(a1[j], p.act);
#pragma unroll
            for (int o = 0; o < MLP_OUT; o++) out[o] = w[L::B3 + o];
            mlp_tail<HD, NH, false>(w, a1, p.act, narrow, out, nullptr);
            if (p.oact == DMR_MLP_SIGMOID) {
#pragma unroll
                for (int o = 0; o < MLP_OUT; o++) out[o] = 1.f / (1.f + expf(-out[o]));
            }
        }
        float* __restrict__ yr = y + row * p.Cout;
        if (p.ovec) {
#pragma unroll
            for (int q = 0; q < MLP_OUT / 4; q++)
                if (4 * q < p.Cout) *reinterpret_cast<float4*>(yr + 4 * q) = make_float4(out[4 * q], out[4 * q + 1], out[4 * q + 2], out[4 * q + 3]);
        } else {
#pragma unroll
            for (int o = 0; o < MLP_OUT; o++)
                if (o < p.Cout) yr[o] = out[o];
        }
    }
}

// ---------------------------------------------------------------------------
// backward.  Per tile a wave recomputes the forward for its 64 rows, runs the layers back per lane for dL/dx, and sums the
// weight gradients dL/dW = sum_rows dz (x) a over its rows: the wave's `a` (64 x in) and `dz` (64 x out) go to its staging
// area in LDS, every lane owns a BO x BI block of the (out, in) entries, sums it over the 64 rows in registers and adds the
// sums to the workgroup's f32 table in LDS (ds_add_f32), which has the weights' layout.  The table leaves once per workgroup,
// to the workgroup's slice of `scratch`; k_mlp_reduce sums the slices in f64 and writes the gradients.
// The staging areas are per wave and a wave is in lockstep: no workgroup barrier inside the tile loop.
// ---------------------------------------------------------------------------
// tbl[o so + i si] += sum_r D[r][o] A[r][i], NO x NI entries over the wave's 64 lanes
template <int NO, int NI, int PD, int PA>
__device__ __forceinline__ void mlp_outer(const float* __restrict__ D, const float* __restrict__ A, float* __restrict__ tbl, int so, int si, int lane) {
    constexpr int PER = NO * NI / 64, BI = PER == 64 ? 8 : (PER >= 4 ? 4 : PER), BO = PER / BI, NIB = NI / BI;
    static_assert(PER * 64 == NO * NI && BO * BI == PER && (NO / BO) * NIB == 64, "a block per lane");
    const int ib = lane % NIB, ob = lane / NIB;
    float acc[BO][BI];
#pragma unroll
    for (int o = 0; o < BO; o++)
#pragma unroll
        for (int i = 0; i < BI; i++) acc[o][i] = 0.f;
    const float* __restrict__ d = D + ob * BO;
    const float* __restrict__ a = A + ib * BI;
#pragma unroll 4
    for (int r = 0; r < 64; r++) {
        float dv[BO], av[BI];
#pragma unroll
        for (int o = 0; o < BO; o++) dv[o] = d[r * PD + o];
#pragma unroll
        for (int i = 0; i < BI; i++) av[i] = a[r * PA + i];
#pragma unroll
        for (int o = 0; o < BO; o++)
#pragma unroll
            for (int i = 0; i < BI; i++) acc[o][i] += dv[o] * av[i];
    }
#pragma unroll
    for (int o = 0; o < BO; o++)
#pragma unroll
        for (int i = 0; i < BI; i++) unsafeAtomicAdd(&tbl[(ob * BO + o) * so + (ib * BI + i) * si], acc[o][i]);
}
// tbl[o] += sum_r D[r][o]
template <int NO, int PD>
__device__ __forceinline__ void mlp_colsum(const float* __restrict__ D, float* __restrict__ tbl, int lane) {
    if (lane < NO) {
        float s = 0.f;
#pragma unroll 8
        for (int r = 0; r < 64; r++) s += D[r * PD + lane];
        unsafeAtomicAdd(&tbl[lane], s);
    }
}
// sum_o wo[o] g[o] over the MLP_OUT padded outputs, or the first four when Cout <= 4 (uniform)
__device__ __forceinline__ float mlp_out_dot(const float* __restrict__ wo, const float (&g)[MLP_OUT], bool narrow) {
    float s = 0.f;
    if (narrow) {
#pragma unroll
        for (int o = 0; o < 4; o++) s += wo[o] * g[o];
    } else {
#pragma unroll
        for (int o = 0; o < MLP_OUT; o++) s += wo[o] * g[o];
    }
    return s;
}
// sum_j w1[c][j] dz[j]
template <int HD>
__device__ __forceinline__ float mlp_dx_dot(const float* __restrict__ wr, const float (&dz)[HD]) {
    float s0 = 0.f, s1 = 0.f;
#pragma unroll
    for (int j = 0; j < HD; j += 2) { s0 += wr[j] * dz[j]; s1 += wr[j + 1] * dz[j + 1]; }
    return s0 + s1;
}

template <int HD, int NH, bool VEC>
__global__ void __launch_bounds__(mlp_bwd_threads(HD, NH))
k_mlp_rows_backward(MlpParams p, int tiles, const float* __restrict__ gout, float* __restrict__ dx, int want_w, float* __restrict__ scratch) {
    constexpr int THREADS = mlp_bwd_threads(HD, NH), WAVES = THREADS / 64, PITCH = HD + 4, GP = MLP_OUT + 4;
    using L = MlpLayout<HD, NH>;
    __shared__ alignas(16) float w[L::TOTAL];
    __shared__ alignas(16) float tbl[L::TOTAL];
    __shared__ alignas(16) float stage[WAVES][64 * (NH * PITCH + GP)];
    const int tid = threadIdx.x, lane = tid & 63;
    float* sa = stage[tid >> 6];                    // [64][PITCH]: the first hidden layer's activations
    float* sb = sa + (NH - 1) * 64 * PITCH;         // [64][PITCH]: the second layer's activations, then dz of a hidden layer
                                                    // (one hidden layer: sa again, once dL/dW_out has read the activations)
    float* sg = sb + 64 * PITCH;                    // [64][GP]: dL/d(pre-activation output), then 16 columns of x
    mlp_load_weights<HD, NH, THREADS>(p, w);
    if (want_w)
        for (int e = tid; e < L::TOTAL; e += THREADS) tbl[e] = 0.f;
    __syncthreads();
    const int n = rows_used(p);
    const bool narrow = p.Cout <= 4;
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t row = (int64_t)tile * THREADS + tid;
        const bool active = row < n;
        if (__ballot(active) == 0ull) {  // (wave-uniform) no row of the wave is used: zeros, and nothing for the sums
            if (dx && row < p.N)
                for (int c = 0; c < p.Cin; c++) dx[row * p.Cin + c] = 0.f;
            continue;
        }
        const float* __restrict__ xr = p.x + row * p.Cin;  // (read by active lanes only; an inactive lane runs on x = 0, upstream 0)
        float a1[HD];
#pragma unroll
        for (int j = 0; j < HD; j++) a1[j] = w[L::B1 + j];
        if (active) mlp_layer_in<HD, VEC>(w + L::W1, xr, p.Cin, a1);
        float out[MLP_OUT];
#pragma unroll
        for (int j = 0; j < HD; j++) { a1[j] = mlp_act(a1[j], p.act); sa[lane * PITCH + j] = a1[j]; }
#pragma unroll
        for (int o = 0; o < MLP_OUT; o++) out[o] = w[L::B3 + o];
        mlp_tail<HD, NH, true>(w, a1, p.act, narrow, out, sb + lane * PITCH);
        float g[MLP_OUT];  // dL/d(pre-activation output): an exact 0 past Cout and in a lane without a row
        {
            const float* __restrict__ gr = gout + row * p.Cout;
#pragma unroll
            for (int o = 0; o < MLP_OUT; o++) g[o] = 0.f;
            if (active) {
                if (p.ovec) {
#pragma unroll
                    for (int q = 0; q < MLP_OUT / 4; q++)
                        if (4 * q < p.Cout) {
                            const float4 t = *reinterpret_cast<const float4*>(gr + 4 * q);
                            g[4 * q] = t.x; g[4 * q + 1] = t.y; g[4 * q + 2] = t.z; g[4 * q + 3] = t.w;
                        }
                } else {
#pragma unroll
                    for (int o = 0; o < MLP_OUT; o++)
                        if (o < p.Cout) g[o] = gr[o];
                }
                if (p.oact == DMR_MLP_SIGMOID) {
#pragma unroll
                    for (int o = 0; o < MLP_OUT; o++) {
                        const float s = 1.f / (1.f + expf(-out[o]));
                        g[o] = o < p.Cout ? g[o] * (s * (1.f - s)) : 0.f;
                    }
                }
            }
#pragma unroll
            for (int o = 0; o < MLP_OUT; o++) sg[lane * GP + o] = g[o];
        }
        rows_wave_sync();
        if (want_w) {  // dL/dW_out, dL/db_out
            if (narrow) mlp_outer<4, HD, GP, PITCH>(sg, sb, tbl + L::W3, 1, MLP_OUT, lane);
            else mlp_outer<MLP_OUT, HD, GP, PITCH>(sg, sb, tbl + L::W3, 1, MLP_OUT, lane);
            mlp_colsum<MLP_OUT, GP>(sg, tbl + L::B3, lane);
            rows_wave_sync();
        }
        float dz1[HD];
        if constexpr (NH == 2) {
            float da1[HD];
#pragma unroll
            for (int i = 0; i < HD; i++) da1[i] = 0.f;
#pragma unroll 2
            for (int j2 = 0; j2 < HD; j2++) {  // dz2 takes a2's place in the lane's row of sb
                const float* __restrict__ wo = w + L::W3 + j2 * MLP_OUT;
                const float da2 = mlp_out_dot(wo, g, narrow);
                const float dz2 = da2 * mlp_dact(sb[lane * PITCH + j2], p.act);
                sb[lane * PITCH + j2] = dz2;
                const float* __restrict__ wr = w + L::W2 + j2 * HD;
#pragma unroll
                for (int i = 0; i < HD; i++) da1[i] += wr[i] * dz2;
            }
            rows_wave_sync();
            if (want_w) {  // dL/dW_mid, dL/db_mid
                mlp_outer<HD, HD, PITCH, PITCH>(sb, sa, tbl + L::W2, HD, 1, lane);
                mlp_colsum<HD, PITCH>(sb, tbl + L::B2, lane);
            }
#pragma unroll
            for (int i = 0; i < HD; i++) dz1[i] = da1[i] * mlp_dact(sa[lane * PITCH + i], p.act);
            rows_wave_sync();
        } else {
#pragma unroll
            for (int j = 0; j < HD; j++) {
                const float* __restrict__ wo = w + L::W3 + j * MLP_OUT;
                dz1[j] = mlp_out_dot(wo, g, narrow) * mlp_dact(a1[j], p.act);
                if (j % 2 == 1) mlp_keep_order();
            }
        }
        if (dx && row < p.N) {  // dL/dx = W_in^T dz1, c by c: a dot product with one row of the W1 image
            float* __restrict__ dr = dx + row * p.Cin;
            if (!active) {
                for (int c = 0; c < p.Cin; c++) dr[c] = 0.f;
            } else if constexpr (VEC) {
                for (int c = 0; c < p.Cin; c += 4) {
                    const float* __restrict__ wr = w + L::W1 + c * HD;
                    *reinterpret_cast<float4*>(dr + c) = make_float4(mlp_dx_dot<HD>(wr, dz1), mlp_dx_dot<HD>(wr + HD, dz1), mlp_dx_dot<HD>(wr + 2 * HD, dz1),
                                                                      mlp_dx_dot<HD>(wr + 3 * HD, dz1));
                }
            } else {
                for (int c = 0; c < p.Cin; c++) dr[c] = mlp_dx_dot<HD>(w + L::W1 + c * HD, dz1);
            }
        }
        if (want_w) {  // dL/dW_in, dL/db_in: dz1 in sb, x through sg sixteen columns at a time
#pragma unroll
            for (int j = 0; j < HD; j++) sb[lane * PITCH + j] = dz1[j];
            rows_wave_sync();
            mlp_colsum<HD, PITCH>(sb, tbl + L::B1, lane);
            for (int c0 = 0; c0 < p.Cin; c0 += MLP_OUT) {
#pragma unroll
                for (int i = 0; i < MLP_OUT; i++) sg[lane * GP + i] = (active && c0 + i < p.Cin) ? xr[c0 + i] : 0.f;
                rows_wave_sync();
                mlp_outer<HD, MLP_OUT, PITCH, GP>(sb, sg, tbl + L::W1 + c0 * HD, 1, HD, lane);
                rows_wave_sync();
            }
        }
        rows_wave_sync();
    }
    if (want_w) {
        __syncthreads();
        float* __restrict__ mine = scratch + (int64_t)blockIdx.x * L::TOTAL;
        for (int e = tid; e < L::TOTAL; e += THREADS) mine[e] = tbl[e];
    }
}

// The workgroups' tables -> the gradients, summed in f64: 64 entries per workgroup, four lanes' partial sums per entry.
// Every wanted output is written whole (groups == 0: zeros); entries of the images' padding go nowhere.
template <int HD, int NH>
__global__ void __launch_bounds__(256)
k_mlp_reduce(const float* __restrict__ scratch, int groups, int Cin, int Cout, float* __restrict__ dw_in, float* __restrict__ db_in,
             float* __restrict__ dw_mid, float* __restrict__ db_mid, float* __restrict__ dw_out, float* __restrict__ db_out) {
    using L = MlpLayout<HD, NH>;
    const int tid = threadIdx.x, e = (int)blockIdx.x * 64 + (tid & 63), part = tid >> 6;
    __shared__ double parts[4][64];
    double s = 0.0;
    if (e < L::TOTAL)
        for (int g = part; g < groups; g += 4) s += (double)scratch[(int64_t)g * L::TOTAL + e];
    parts[part][tid & 63] = s;
    __syncthreads();
    if (part != 0 || e >= L::TOTAL) return;
    const float v = (float)(parts[0][tid] + parts[1][tid] + parts[2][tid] + parts[3][tid]);
    if (e < L::B1) { const int c = e / HD, j = e % HD; if (dw_in && c < Cin) dw_in[j * Cin + c] = v; }
    else if (e < L::W2) { if (db_in) db_in[e - L::B1] = v; }
    else if (e < L::B2) { if (dw_mid) dw_mid[e - L::W2] = v; }
    else if (e < L::W3) { if (db_mid) db_mid[e - L::B2] = v; }
    else if (e < L::B3) { const int j = (e - L::W3) / MLP_OUT, o = (e - L::W3) % MLP_OUT; if (dw_out && o < Cout) dw_out[o * HD + j] = v; }
    else { const int o = e - L::B3; if (db_out && o < Cout) db_out[o] = v; }
}

#pragma clang fp contract(off)

// f(Hd, hidden layers, float4 row loads) as integral constants: the 12 instantiations of each kernel
template <class Fn>
void mlp_with_shape(int Hd, int n_hidden, bool vec, Fn&& f) {
    with_one_of<16, 32, 64>(Hd, [&](auto hd) {
        with_one_of<1, 2>(n_hidden, [&](auto nh) {
            if (vec) f(hd, nh, std::true_type());
            else f(hd, nh, std::false_type());
        });
    });
}

// what both calls check first, in the header's order -> MlpParams
int mlp_params(const char* name, int N, int Cin, int Hd, int Cout, int n_hidden, int act, int oact, const float* x, const float* W_in,
               const float* b_in, const float* W_mid, const float* b_mid, const float* W_out, const float* b_out, const int32_t* n_rows,
               MlpParams& p) {
    const std::string n = std::string(name) + ": ";
    if (N < 0) return api_fail((n + "bad rows").c_str());
    if (Hd != 16 && Hd != 32 && Hd != 64) return api_fail((n + "Hd must be 16, 32 or 64, got " + std::to_string(Hd)).c_str());
    if (Cin < 1 || Cin > MLP_MAX_CIN) return api_fail((n + "Cin must be in 1.." + std::to_string(MLP_MAX_CIN) + ", got " + std::to_string(Cin)).c_str());
    if (Cout < 1 || Cout > MLP_OUT) return api_fail((n + "Cout must be in 1.." + std::to_string(MLP_OUT) + ", got " + std::to_string(Cout)).c_str());
    if (n_hidden != 1 && n_hidden != 2) return api_fail((n + "n_hidden must be 1 or 2, got " + std::to_string(n_hidden)).c_str());
    if ((act != DMR_MLP_RELU && act != DMR_MLP_TANH) || (oact != DMR_MLP_NONE && oact != DMR_MLP_SIGMOID)) return api_fail((n + "bad activation").c_str());
    if (N > 0 && !x) return api_fail((n + "null x").c_str());
    if (!W_in || !W_out || (n_hidden == 2 && !W_mid)) return api_fail((n + "null weights").c_str());
    p.N = N; p.Cin = Cin; p.Cout = Cout; p.act = act; p.oact = oact; p.ovec = 0;
    p.x = x; p.w_in = W_in; p.b_in = b_in; p.w_mid = n_hidden == 2 ? W_mid : nullptr; p.b_mid = n_hidden == 2 ? b_mid : nullptr;
    p.w_out = W_out; p.b_out = b_out; p.n_rows = n_rows;
    return 0;
}

}  // namespace
}  // namespace dmr

extern "C" {

int dmr_mlp_rows(int N, int Cin, int Hd, int Cout, int n_hidden, int act, int oact, const float* x, const float* W_in,
                 const float* b_in, const float* W_mid, const float* b_mid, const float* W_out, const float* b_out,
                 const int32_t* n_rows, float* y, void* stream) {
    using namespace dmr;
    const char* name = "dmr_mlp_rows";
    MlpParams p;
    if (mlp_params(name, N, Cin, Hd, Cout, n_hidden, act, oact, x, W_in, b_in, W_mid, b_mid, W_out, b_out, n_rows, p)) return 1;
    if (N == 0) return 0;
    if (!y) return api_fail("dmr_mlp_rows: null output");
    p.ovec = shade_vec(Cout, y);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const RowsGrid g = rows_grid(N, MLP_FWD_THREADS, MLP_FWD_MAX_GROUPS);
    const dim3 groups((unsigned)g.groups), block(MLP_FWD_THREADS);
    mlp_with_shape(Hd, n_hidden, shade_vec(Cin, x) != 0, [&](auto hd, auto nh, auto vec) {
        k_mlp_rows<decltype(hd)::value, decltype(nh)::value, decltype(vec)::value><<<groups, block, 0, st>>>(p, g.tiles, y);
    });
    return launched(name);
}

int dmr_mlp_rows_backward(int N, int Cin, int Hd, int Cout, int n_hidden, int act, int oact, const float* x, const float* W_in,
                          const float* b_in, const float* W_mid, const float* b_mid, const float* W_out, const float* b_out,
                          const int32_t* n_rows, const float* grad_out, float* dL_dx, float* dL_dW_in, float* dL_db_in,
                          float* dL_dW_mid, float* dL_db_mid, float* dL_dW_out, float* dL_db_out, float* scratch,
                          int64_t scratch_floats, void* stream) {
    using namespace dmr;
    const char* name = "dmr_mlp_rows_backward";
    MlpParams p;
    if (mlp_params(name, N, Cin, Hd, Cout, n_hidden, act, oact, x, W_in, b_in, W_mid, b_mid, W_out, b_out, n_rows, p)) return 1;
    const char* own = nullptr;
    if ((dL_dW_mid || dL_db_mid) && n_hidden != 2) own = "a gradient of the second hidden layer without one";
    else if ((dL_db_in && !b_in) || (dL_db_mid && !b_mid) || (dL_db_out && !b_out)) own = "the gradient of a bias without the bias";
    const bool want_w = dL_dW_in || dL_db_in || dL_dW_mid || dL_db_mid || dL_dW_out || dL_db_out;
    const int go = rows_backward_prologue(name, N, grad_out, own, dL_dx, want_w);
    if (go != SHADE_LAUNCH) return go;
    if (want_w && (!scratch || scratch_floats < DMR_MLP_SCRATCH_FLOATS(Hd, n_hidden))) return api_fail("dmr_mlp_rows_backward: scratch too small");
    p.ovec = shade_vec(Cout, grad_out);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const RowsGrid g = rows_grid(N, mlp_bwd_threads(Hd, n_hidden), MLP_BWD_MAX_GROUPS);
    const bool vec = shade_vec(Cin, x) && (!dL_dx || shade_vec(Cin, dL_dx));
    mlp_with_shape(Hd, n_hidden, vec, [&](auto hd, auto nh, auto v) {
        constexpr int HD = decltype(hd)::value, NH = decltype(nh)::value;
        if (g.groups > 0)
            k_mlp_rows_backward<HD, NH, decltype(v)::value><<<dim3((unsigned)g.groups), dim3(mlp_bwd_threads(HD, NH)), 0, st>>>(p, g.tiles, grad_out, dL_dx,
                                                                                                                         want_w ? 1 : 0, scratch);
        if (want_w)
            k_mlp_reduce<HD, NH><<<dim3((unsigned)((MlpLayout<HD, NH>::TOTAL + 63) / 64)), dim3(256), 0, st>>>(scratch, g.groups, Cin, Cout, dL_dW_in, dL_db_in,
                                                                                                            dL_dW_mid, dL_db_mid, dL_dW_out, dL_db_out);
    });
    return launched(name);
}

}  // extern "C"
