/* dmesh_renderer_amd_mlp.h -- a small MLP over packed, channel-last rows: the neural shader between the two ends of
 * dmesh_renderer_amd_packed.h, as one forward and one backward kernel.
 *
 * A companion of dmesh_renderer_amd.h (same library, libdmesh_renderer_hip.so; errors are read through its
 * dmr_last_error()).  No dmr_scene and no fragment lists: the calls see rows only.
 *
 *   n_hidden = 1    y = oact(W_out act(W_in x + b_in) + b_out)
 *   n_hidden = 2    y = oact(W_out act(W_mid act(W_in x + b_in) + b_mid) + b_out)
 *
 * x f32 [N,Cin], W_in f32 [Hd,Cin], W_mid f32 [Hd,Hd] (n_hidden = 2 only; ignored and may be null otherwise), W_out f32 [Cout,Hd]:
 * row-major, out x in, the layout of a linear layer's weight.  b_in [Hd], b_mid [Hd], b_out [Cout]: each may be null (no bias).
 * y f32 [N,Cout].  act: DMR_MLP_RELU or DMR_MLP_TANH (the derivative of relu at exactly 0 is 0); oact: DMR_MLP_NONE or
 * DMR_MLP_SIGMOID.  Hd in {16, 32, 64}, 1 <= Cin <= 64, 1 <= Cout <= 16, 0 <= N < 2^31.  Offsets into the [N,C] buffers are
 * 64-bit.
 *
 * n_rows i32 [1] on the device, or null (= N): rows r >= min(max(n_rows[0], 0), N) are NOT READ, in x and in grad_out; they get
 * exact zeros in y and in dL_dx and add nothing to any weight or bias gradient.  The count is read on the device.
 *
 * The hidden activations never reach memory: the backward takes x, the weights and grad_out and recomputes them.  Nothing of
 * size [N,Hd] is stored by either call.
 *
 * Both calls only enqueue on `stream`: no host wait, no allocation, safe to capture into a HIP graph.  Every output is fully
 * overwritten (no memset node: the weight gradients are written by a kernel that sums the workgroups' partial sums in f64).
 * All pointers are device pointers.  Return value: 0 on success, non-zero on error; dmr_last_error() then returns a
 * description.  The first check that fails decides it, in this order: "bad rows" (N below 0), Hd, Cin, Cout, n_hidden, the
 * activations, null x (when N > 0), null weights (W_in, W_out, and W_mid when n_hidden = 2) -- and only then what a single
 * call asks for: a null output (when N > 0), a null grad_out (when N > 0), a weight or bias gradient of a tensor that was not
 * given, a scratch buffer that is null or too small (when a weight or bias gradient is wanted).
 */
#ifndef DMESH_RENDERER_AMD_MLP_H
#define DMESH_RENDERER_AMD_MLP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DMR_MLP_RELU 0
#define DMR_MLP_TANH 1
#define DMR_MLP_NONE 0
#define DMR_MLP_SIGMOID 1

/* The backward's workgroups leave their partial weight-gradient sums in `scratch`, which the caller provides:
 * DMR_MLP_SCRATCH_FLOATS(Hd, n_hidden) floats (at most 19 169 280 bytes), whatever N, Cin and Cout.  Its contents mean
 * nothing before or after the call. */
#define DMR_MLP_MAX_GROUPS 512
#define DMR_MLP_TABLE_FLOATS(Hd, n_hidden) (64 * (Hd) + (Hd) + ((n_hidden) == 2 ? (Hd) * (Hd) + (Hd) : 0) + 16 * (Hd) + 16)
#define DMR_MLP_SCRATCH_FLOATS(Hd, n_hidden) ((int64_t)DMR_MLP_MAX_GROUPS * DMR_MLP_TABLE_FLOATS(Hd, n_hidden))

/* -> y f32 [N,Cout].  N == 0: returns 0 and enqueues nothing. */
int dmr_mlp_rows(int N, int Cin, int Hd, int Cout, int n_hidden, int act, int oact, const float* x, const float* W_in,
                 const float* b_in, const float* W_mid, const float* b_mid, const float* W_out, const float* b_out,
                 const int32_t* n_rows, float* y, void* stream);

/* The gradients of y.  grad_out f32 [N,Cout] is the upstream gradient.  Each of the seven outputs may be null (not wanted, and
 * then not computed): dL_dx f32 [N,Cin], and the gradients of the weights and biases in their own shapes (dL_dW_mid / dL_db_mid
 * need n_hidden = 2, a bias gradient needs its bias).  With no output wanted the call returns 0 and enqueues nothing.  N == 0:
 * the weight and bias gradients that were asked for are written as zeros (one launch), nothing else is enqueued. */
int dmr_mlp_rows_backward(int N, int Cin, int Hd, int Cout, int n_hidden, int act, int oact, const float* x, const float* W_in,
                          const float* b_in, const float* W_mid, const float* b_mid, const float* W_out, const float* b_out,
                          const int32_t* n_rows, const float* grad_out, float* dL_dx, float* dL_dW_in, float* dL_db_in,
                          float* dL_dW_mid, float* dL_db_mid, float* dL_dW_out, float* dL_db_out, float* scratch,
                          int64_t scratch_floats, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DMESH_RENDERER_AMD_MLP_H */
