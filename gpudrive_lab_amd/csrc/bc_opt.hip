// Device BC update (gd_bc_train_rows, gd_bc_adamw, gd_bc_adamw_dim): what stands between gd_bc_forward and gd_bc_backward, and after the
// backward, in one gradient step of the reference's imitation learning -- the step's statistics and the loss's upstream
// gradient, gradient clipping, the largest per-tensor norm and AdamW.  The rule is csrc/bc_opt_rule.hpp, stated there in full;
// these kernels only distribute it:
//   k_bc_rows    ONE workgroup of 256 lanes.  Lane j owns partial j of every sum and walks the rows j, j + 256, ..; the
//                partials meet in LDS and lanes 0..3 add one statistic's each in ascending order.  grad_nll is stored per row.
//   k_bc_sq      a workgroup of 256 lanes per parameter TENSOR: the tensor's sum of squares by the same order (lane j owns
//                partial j, counted from the tensor's start), left as float64 in `scal` with its root in tensor_norms.  The
//                largest tensor is head.input_layer.0.weight: 12,288 floats at network_dim 64, a lane's 48 elements; 24,576 at
//                128, a lane's 96.
//   k_bc_step    ONE workgroup: the sums of the launch before it added in ascending tensor order, the norm, the coefficient,
//                the largest tensor norm; lane 0 advances step and the two running products and leaves total, coef, bc1 and
//                rbc2 in `scal` for the next launch.
//   k_bc_adamw   a lane per parameter: the AdamW rule, the updated weight stored to params[e] and to blob[blob_of[e]].  It
//                reads the scalars of the launch before it and writes none.
// No atomics, no word crosses workgroups within a launch, every store has one owner: equal inputs and state give equal bits.
// None of them has the policy's width in it: G, T, tensor_end and blob_of carry the layout, and T <= MAX_TENSORS = 288 at either
// width (the sweep's model at network_dim 128, layers (4, 3): G = 1,399,274, T = 252; indices stay far below 2^31).
// All four are short latency chains or one sweep over G floats (0.3 M at 64, 1.4 M at 128): 256-lane workgroups, a few KB of LDS,
// no scratch.
#include <hip/hip_runtime.h>

#include "bc_opt_rule.hpp"
#include "engine.hpp"

namespace gd {

namespace {

namespace R = bc_opt_rule;
namespace P = ppo_rule;
constexpr int NT = R::LANES;
constexpr int SCAL_FLOATS = 4;  // total, coef, bc1, rbc2; the tensors' float64 sums follow

__global__ __launch_bounds__(NT) void k_bc_rows(int n, float scale, const float *__restrict__ nll, const float *__restrict__ actions,
                                                const float *__restrict__ expert, float *__restrict__ grad_nll,
                                                float *__restrict__ stats, float *__restrict__ stats_sum) {
    __shared__ double s_part[4][NT];
    const int lane = threadIdx.x;
    const float w = R::grad_nll_of(n);
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = lane; i < n; i += NT) {
        acc[0] += (double)nll[i];
#pragma unroll
        for (int d = 0; d < 3; d++) acc[1 + d] += (double)R::abs_error(actions[3 * (size_t)i + d], expert[3 * (size_t)i + d]);
        grad_nll[i] = w;
    }
#pragma unroll
    for (int k = 0; k < 4; k++) s_part[k][lane] = acc[k];
    __syncthreads();
    if (lane < 4) {
        double t = 0.0;
        for (int j = 0; j < NT; j++) t += s_part[lane][j];
        const float v = R::mean_of(t, n);
        stats[lane] = v;
        stats_sum[lane] = stats_sum[lane] + scale * v;
    }
}

__global__ __launch_bounds__(NT) void k_bc_sq(int total, int num_tensors, const int32_t *__restrict__ tensor_end,
                                              const float *__restrict__ grad, double *__restrict__ sq,
                                              float *__restrict__ tensor_norms) {
    __shared__ double s_part[NT];
    const int t = blockIdx.x;
    if (t >= num_tensors) return;
    // (memory safety: a range outside the gradient is cut to it; the layout's ranges never are)
    int lo = t ? tensor_end[t - 1] : 0, hi = tensor_end[t];
    lo = min(max(lo, 0), total), hi = min(max(hi, lo), total);
    double acc = 0.0;
    for (int e = lo + (int)threadIdx.x; e < hi; e += NT) acc += (double)R::square(grad[e]);
    s_part[threadIdx.x] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int j = 0; j < NT; j++) s += s_part[j];
        sq[t] = s;
        tensor_norms[t] = R::tensor_norm(s);
    }
}

__global__ __launch_bounds__(NT) void k_bc_step(int num_tensors, float max_norm, double beta1, double beta2, float scale,
                                                const double *__restrict__ sq, const float *__restrict__ tensor_norms,
                                                int32_t *__restrict__ step, double *__restrict__ beta_pow, float *__restrict__ scal,
                                                float *__restrict__ stats, float *__restrict__ stats_sum,
                                                int32_t *__restrict__ max_grad_tensor) {
    __shared__ double s_sq[R::MAX_TENSORS];
    __shared__ float s_norm[R::MAX_TENSORS];
    for (int t = threadIdx.x; t < num_tensors; t += NT) s_sq[t] = sq[t], s_norm[t] = tensor_norms[t];
    __syncthreads();
    if (threadIdx.x == 0) {
        double sum_sq = 0.0;
        for (int t = 0; t < num_tensors; t++) sum_sq += s_sq[t];
        const double pow1 = beta_pow[0] * beta1, pow2 = beta_pow[1] * beta2;
        beta_pow[0] = pow1, beta_pow[1] = pow2;
        step[0] = step[0] + 1;
        const P::StepScalars s = P::step_scalars(sum_sq, max_norm, pow1, pow2);
        const R::MaxNorm mx = R::max_norm_of(s_norm, num_tensors, s.coef);
        scal[0] = s.total, scal[1] = s.coef, scal[2] = s.bc1, scal[3] = s.rbc2;
        stats[R::GRAD_NORM] = s.total, stats[R::MAX_GRAD_NORM] = mx.value;
        stats_sum[R::GRAD_NORM] = stats_sum[R::GRAD_NORM] + scale * s.total;
        stats_sum[R::MAX_GRAD_NORM] = stats_sum[R::MAX_GRAD_NORM] + scale * mx.value;
        max_grad_tensor[0] = mx.tensor;
    }
}

__global__ __launch_bounds__(NT) void k_bc_adamw(int total, long long blob_floats, P::AdamCoefs c, float weight_decay,
                                                 const float *__restrict__ lr, const float *__restrict__ scal,
                                                 const float *__restrict__ grad, const int32_t *__restrict__ blob_of,
                                                 float *__restrict__ params, float *__restrict__ exp_avg,
                                                 float *__restrict__ exp_avg_sq, float *__restrict__ blob) {
    const int e = blockIdx.x * NT + threadIdx.x;
    if (e >= total) return;
    const P::StepScalars s{scal[0], scal[1], scal[2], scal[3]};
    const float rate = lr[0];
    float p = params[e], m = exp_avg[e], v = exp_avg_sq[e];
    R::adamw(c, s, rate, R::decay_of(rate, weight_decay), grad[e], p, m, v);
    params[e] = p, exp_avg[e] = m, exp_avg_sq[e] = v;
    const long long at = blob_of[e];
    if (at >= 0 && at < blob_floats) blob[at] = p;  // (memory safety: the inverse of the layout is always inside the blob)
}

}  // namespace

int bc_num_tensors(int fusion_layers, int branch_layers, int head_layers) {
    // three embedders of 4 x (Linear, LayerNorm); self-attention layers of 16 tensors; two cross layers of 18; the head
    return 48 + 16 * (fusion_layers + 2 * branch_layers) + 36 + 2 * (head_layers + 2);
}

void launch_bc_train_rows(const gd_bc_opt &o, hipStream_t st, int n, const float *nll, const float *actions,
                          const float *expert_actions, float *grad_nll) {
    hipLaunchKernelGGL(k_bc_rows, dim3(1), dim3(NT), 0, st, n, o.stats_scale, nll, actions, expert_actions, grad_nll, o.stats,
                       o.stats_sum);
}

void launch_bc_adamw(const gd_bc_opt &o, hipStream_t st, const float *grad) {
    const int total = (int)o.grad_floats, T = o.num_tensors;
    double *sq = reinterpret_cast<double *>(o.scal + SCAL_FLOATS);
    hipLaunchKernelGGL(k_bc_sq, dim3((unsigned)T), dim3(NT), 0, st, total, T, o.tensor_end, grad, sq, o.tensor_norms);
    hipLaunchKernelGGL(k_bc_step, dim3(1), dim3(NT), 0, st, T, o.max_grad_norm, o.beta1, o.beta2, o.stats_scale, sq, o.tensor_norms,
                       o.step, o.beta_pow, o.scal, o.stats, o.stats_sum, o.max_grad_tensor);
    hipLaunchKernelGGL(k_bc_adamw, dim3((unsigned)((total + NT - 1) / NT)), dim3(NT), 0, st, total, (long long)o.blob_floats,
                       P::adam_coefs(o.beta1, o.beta2, o.eps), o.weight_decay, o.lr, o.scal, grad, o.blob_of, o.params, o.exp_avg,
                       o.exp_avg_sq, o.blob);
}

}  // namespace gd
