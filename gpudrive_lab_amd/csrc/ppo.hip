// Device PPO update (gd_ppo_loss, gd_ppo_adam): what stands between gd_policy_evaluate and gd_policy_backward, and after the
// backward, in one minibatch update -- the reference's loss and its three upstream gradients, gradient clipping and Adam.
// The rule is csrc/ppo_rule.hpp, stated there in full; these kernels only distribute it:
//   k_ppo_loss   ONE workgroup of 256 lanes.  Every sum of the rule is "element i to partial i mod 256 in ascending i", so lane
//                j owns partial j and walks the rows j, j + 256, ..; the 256 partials meet in LDS and are added in ascending
//                order.  Three walks over the rows: the advantages' mean, their variance (both skipped without norm_adv), then
//                the row rule -- the three upstream gradients stored, the six statistics' terms summed.  Lanes 0..5 finish one
//                statistic each.  At the reference's minibatch of 8,192 a lane has 32 rows.
//   k_ppo_norm   ONE workgroup: the gradient's sum of squares by the same order, then lane 0 advances step and the two running
//                products and leaves total, coef, bc1 and rbc2 in `scal` for the next launch.
//   k_ppo_adam   a lane per parameter: the Adam rule, the updated weight stored to params[e] and to blob[blob_of[e]].  It reads
//                the scalars of the launch before it and writes none.
// No atomics, no scalar crosses workgroups within a launch, every store has one owner: equal inputs and state give equal bits.
#include <hip/hip_runtime.h>

#include "engine.hpp"
#include "ppo_rule.hpp"

namespace gd {

namespace {

namespace R = ppo_rule;
constexpr int NT = R::LANES;

// the 256 partials, added in ascending order; every lane returns the same sum.  The barrier in front lets s be reused.
__device__ __forceinline__ double ordered_total(double *s, double mine) {
    __syncthreads();
    s[threadIdx.x] = mine;
    __syncthreads();
    double t = 0.0;
    for (int j = 0; j < NT; j++) t += s[j];
    return t;
}

__global__ __launch_bounds__(NT) void k_ppo_loss(R::Hyper h, int m, float scale, const float *__restrict__ newlogprob,
                                                 const float *__restrict__ entropy, const float *__restrict__ newvalue,
                                                 const float *__restrict__ old_logprob, const float *__restrict__ old_value,
                                                 const float *__restrict__ adv, const float *__restrict__ ret,
                                                 float *__restrict__ d_logprob, float *__restrict__ d_entropy,
                                                 float *__restrict__ d_value, float *__restrict__ stats,
                                                 float *__restrict__ stats_sum) {
    __shared__ double s_part[6][NT];
    const int lane = threadIdx.x;
    R::Norm nm{0.f, 1.f};
    if (h.norm_adv) {
        double acc = 0.0;
        for (int i = lane; i < m; i += NT) acc += (double)adv[i];
        const float mean = R::mean_of(ordered_total(s_part[0], acc), m);
        acc = 0.0;
        for (int i = lane; i < m; i += NT) acc += (double)R::centred_square(adv[i], mean);
        nm = R::norm_of(mean, ordered_total(s_part[0], acc), m);
    }
    const float inv_m = 1.f / (float)m;
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = lane; i < m; i += NT) {
        const float ent = entropy[i];
        const R::Row r = R::row(h, nm, inv_m, newlogprob[i], newvalue[i], old_logprob[i], old_value[i], adv[i], ret[i]);
        d_logprob[i] = r.d_logprob, d_entropy[i] = r.d_entropy, d_value[i] = r.d_value;
        acc[R::POLICY_LOSS] += (double)r.pg, acc[R::VALUE_LOSS] += (double)r.vl, acc[R::ENTROPY] += (double)ent;
        acc[R::OLD_APPROX_KL] += (double)r.neg_logratio, acc[R::APPROX_KL] += (double)r.kl, acc[R::CLIPFRAC] += (double)r.clipped;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 6; k++) s_part[k][lane] = acc[k];
    __syncthreads();
    if (lane < 6) {
        double t = 0.0;
        for (int j = 0; j < NT; j++) t += s_part[lane][j];
        float v = R::mean_of(t, m);
        if (lane == R::VALUE_LOSS) v = 0.5f * v;
        stats[lane] = v;
        stats_sum[lane] = stats_sum[lane] + scale * v;
    }
}

__global__ __launch_bounds__(NT) void k_ppo_norm(int total, float max_norm, double beta1, double beta2, float scale,
                                                 const float *__restrict__ grad, int32_t *__restrict__ step,
                                                 double *__restrict__ beta_pow, float *__restrict__ scal,
                                                 float *__restrict__ stats, float *__restrict__ stats_sum) {
    __shared__ double s_part[NT];
    double acc = 0.0;
    for (int e = threadIdx.x; e < total; e += NT) {
        const float g = grad[e];
        acc += (double)(g * g);
    }
    const double sum_sq = ordered_total(s_part, acc);
    if (threadIdx.x == 0) {
        const double pow1 = beta_pow[0] * beta1, pow2 = beta_pow[1] * beta2;
        beta_pow[0] = pow1, beta_pow[1] = pow2;
        step[0] = step[0] + 1;
        const R::StepScalars s = R::step_scalars(sum_sq, max_norm, pow1, pow2);
        scal[0] = s.total, scal[1] = s.coef, scal[2] = s.bc1, scal[3] = s.rbc2;
        stats[R::GRAD_NORM] = s.total;
        stats_sum[R::GRAD_NORM] = stats_sum[R::GRAD_NORM] + scale * s.total;
    }
}

__global__ __launch_bounds__(NT) void k_ppo_adam(int total, long long blob_floats, R::AdamCoefs c, const float *__restrict__ lr,
                                                 const float *__restrict__ scal, const float *__restrict__ grad,
                                                 const int32_t *__restrict__ blob_of, float *__restrict__ params,
                                                 float *__restrict__ exp_avg, float *__restrict__ exp_avg_sq,
                                                 float *__restrict__ blob) {
    const int e = blockIdx.x * NT + threadIdx.x;
    if (e >= total) return;
    const R::StepScalars s{scal[0], scal[1], scal[2], scal[3]};
    float p = params[e], m = exp_avg[e], v = exp_avg_sq[e];
    R::adam(c, s, lr[0], grad[e], p, m, v);
    params[e] = p, exp_avg[e] = m, exp_avg_sq[e] = v;
    const long long at = blob_of[e];
    if (at >= 0 && at < blob_floats) blob[at] = p;  // (memory safety: the inverse of the layout is always inside the blob)
}

R::Hyper hyper(const gd_ppo &o) {
    return R::Hyper{o.clip_coef, o.vf_clip_coef, o.ent_coef, o.vf_coef, o.norm_adv != 0, o.clip_vloss != 0};
}

}  // namespace

void launch_ppo_loss(const gd_ppo &o, hipStream_t st, const float *newlogprob, const float *entropy, const float *newvalue,
                     const float *old_logprob, const float *old_value, const float *adv, const float *ret, float *d_logprob,
                     float *d_entropy, float *d_value) {
    hipLaunchKernelGGL(k_ppo_loss, dim3(1), dim3(NT), 0, st, hyper(o), o.num_rows, o.stats_scale, newlogprob, entropy, newvalue,
                       old_logprob, old_value, adv, ret, d_logprob, d_entropy, d_value, o.stats, o.stats_sum);
}

void launch_ppo_adam(const gd_ppo &o, hipStream_t st, const float *grad) {
    const int total = (int)o.grad_floats;
    hipLaunchKernelGGL(k_ppo_norm, dim3(1), dim3(NT), 0, st, total, o.max_grad_norm, o.beta1, o.beta2, o.stats_scale, grad, o.step,
                       o.beta_pow, o.scal, o.stats, o.stats_sum);
    hipLaunchKernelGGL(k_ppo_adam, dim3((unsigned)((total + NT - 1) / NT)), dim3(NT), 0, st, total, (long long)o.blob_floats,
                       R::adam_coefs(o.beta1, o.beta2, o.eps), o.lr, o.scal, grad, o.blob_of, o.params, o.exp_avg, o.exp_avg_sq,
                       o.blob);
}

}  // namespace gd
