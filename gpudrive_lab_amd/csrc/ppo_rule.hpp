// The rule of the device PPO update (ppo.hip: gd_ppo_loss, gd_ppo_adam) as plain C++, so that the device and a host program
// (tests/ppo_rule_host.cpp) run the same arithmetic.  It is the reference's minibatch loss (gpudrive/integrations/puffer/
// ppo.py:282-324), torch.nn.utils.clip_grad_norm_ and torch.optim.Adam (no weight decay, no amsgrad) with every rounding fixed.
//
// ARITHMETIC.  Everything per row and per parameter is float32 and rounds every operation: compile the including unit with
// -ffp-contract=off.  Every SUM over rows or parameters has float32 terms, a float64 accumulator and one order: element i is
// added to partial i mod 256, in ascending i, and then the 256 partials are added in ascending order (ordered_sum below is
// the statement; the device runs it as one workgroup of 256 lanes, lane j owning partial j).
//
// LOSS.  Inputs [M] float32: newlogprob, entropy, newvalue (of gd_policy_evaluate), old logprob, old value, advantage, return.
//     invM = 1.f / (float) M
//     norm_adv:  mean = (float) (SUM adv / (double) M);  d = adv - mean;  var = (float) (SUM (d * d) / (double) (M - 1))
//                (the unbiased variance, torch's .std());  a = (adv - mean) / (sqrtf(var) + 1e-8f).   Otherwise a = adv.
//     logratio = newlogprob - old_logprob;  ratio = expf(logratio)
//     lo = 1.f - clip, hi = 1.f + clip;  rc = fminf(fmaxf(ratio, lo), hi)
//     pg1 = (-a) * ratio;  pg2 = (-a) * rc;  pg = fmaxf(pg1, pg2)
//     vu = (newvalue - ret)^2
//     clip_vloss:  dv = newvalue - old_value;  vcl = old_value + fminf(fmaxf(dv, -vclip), vclip);  vc = (vcl - ret)^2;
//                  vl = fmaxf(vu, vc).   Otherwise vl = vu.
//     loss = mean(pg) - ent_coef * mean(entropy) + vf_coef * (0.5 * mean(vl))
// The upstream gradients of that loss, every element stored, follow torch's autograd: an elementwise max hands the gradient to
// the larger branch and HALF to each on a tie; a clamp passes the gradient where its input lies within the bounds, the bounds
// themselves included; a is a constant (no gradient through mean or std).  With w(x, y) = 1 if x > y, 0.5 if x == y, else 0:
//     w1 = w(pg1, pg2);  w2 = (lo <= ratio && ratio <= hi) ? 1.f - w1 : 0.f
//     d_logprob = (((-a) * (w1 + w2)) * invM) * ratio
// so a ratio inside the range or on a bound (pg1 == pg2, w1 + w2 = 1) gives (-a * invM) * ratio, and outside it the unclipped
// branch counts only where it is the larger.
//     d_entropy = -(ent_coef * invM)
//     clip_vloss:  u1 = w(vu, vc);  u2 = (-vclip <= dv && dv <= vclip) ? 1.f - u1 : 0.f
//                  d_value = (vf_coef * (0.5f * invM)) * (u1 * (2.f * (newvalue - ret)) + u2 * (2.f * (vcl - ret)))
//     otherwise    d_value = (vf_coef * (0.5f * invM)) * (2.f * (newvalue - ret))
// The statistics, each (float) (SUM term / (double) M): policy_loss (pg), value_loss (vl, then times 0.5f), entropy,
// old_approx_kl (-logratio), approx_kl ((ratio - 1.f) - logratio), clipfrac (fabsf(ratio - 1.f) > clip ? 1.f : 0.f); the
// seventh, grad_norm, is the optimiser step's `total`.
//
// CLIP AND ADAM.  g [G] is the gradient; beta1, beta2 are float64; pow1, pow2 (float64) and step (int32) are state.
//     total = sqrtf((float) SUM (g * g));  coef = fminf(1.f, max_norm / (total + 1e-6f))
//     step += 1;  pow1 *= beta1;  pow2 *= beta2   (one float64 product per step, no pow(), so host and device agree)
//     bc1 = (float) (1.0 - pow1);  rbc2 = sqrtf((float) (1.0 - pow2));  step_size = lr / bc1
//     omb1 = (float) (1.0 - beta1);  b2 = (float) beta2;  omb2 = (float) (1.0 - beta2)
//     per parameter:  gc = g * coef;  m = m + (gc - m) * omb1;  v = v * b2 + omb2 * (gc * gc)
//                     p = p - step_size * (m / (sqrtf(v) / rbc2 + eps))
// sqrtf and the divisions are correctly rounded on both sides and nothing here is transcendental, so the optimiser step is
// bit-identical between the device and the host program.  A non-finite gradient propagates as in torch.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define GD_PPO_FN __host__ __device__ __forceinline__
#else
#define GD_PPO_FN inline
#endif

namespace gd {
namespace ppo_rule {

constexpr int LANES = 256;
constexpr int N_STATS = 7;
enum { POLICY_LOSS = 0, VALUE_LOSS, ENTROPY, OLD_APPROX_KL, APPROX_KL, CLIPFRAC, GRAD_NORM };

// the statement of every sum: term(i) is float32
template <class Term>
inline double ordered_sum(long long n, Term term) {
    double part[LANES];
    for (int j = 0; j < LANES; j++) part[j] = 0.0;
    for (long long i = 0; i < n; i++) part[i % LANES] += (double)term(i);
    double s = 0.0;
    for (int j = 0; j < LANES; j++) s += part[j];
    return s;
}

struct Hyper {
    float clip_coef, vf_clip_coef, ent_coef, vf_coef;
    bool norm_adv, clip_vloss;
};

struct Norm {
    float mean, denom;  // a = (adv - mean) / denom
};

GD_PPO_FN float mean_of(double sum, int m) { return (float)(sum / (double)m); }
GD_PPO_FN float centred_square(float adv, float mean) {
    const float d = adv - mean;
    return d * d;
}
GD_PPO_FN Norm norm_of(float mean, double sum_sq, int m) { return Norm{mean, sqrtf((float)(sum_sq / (double)(m - 1))) + 1e-8f}; }

struct Row {
    float d_logprob, d_entropy, d_value;
    float pg, vl, neg_logratio, kl, clipped;  // the terms of the statistics' sums; the entropy's term is the input itself
};

GD_PPO_FN float tie_weight(float x, float y) { return x > y ? 1.f : (x == y ? 0.5f : 0.f); }

GD_PPO_FN Row row(const Hyper &h, Norm nm, float inv_m, float newlogprob, float newvalue, float old_logprob, float old_value,
                  float adv, float ret) {
    Row r;
    const float a = h.norm_adv ? (adv - nm.mean) / nm.denom : adv;
    const float logratio = newlogprob - old_logprob;
    const float ratio = expf(logratio);
    const float lo = 1.f - h.clip_coef, hi = 1.f + h.clip_coef;
    const float rc = fminf(fmaxf(ratio, lo), hi);
    const float pg1 = (-a) * ratio, pg2 = (-a) * rc;
    r.pg = fmaxf(pg1, pg2);
    const float w1 = tie_weight(pg1, pg2);
    const float w2 = (lo <= ratio && ratio <= hi) ? 1.f - w1 : 0.f;
    r.d_logprob = (((-a) * (w1 + w2)) * inv_m) * ratio;
    r.d_entropy = -(h.ent_coef * inv_m);
    const float eu = newvalue - ret;
    const float vu = eu * eu;
    const float scale = h.vf_coef * (0.5f * inv_m);
    if (h.clip_vloss) {
        const float dv = newvalue - old_value;
        const float vcl = old_value + fminf(fmaxf(dv, -h.vf_clip_coef), h.vf_clip_coef);
        const float ec = vcl - ret;
        const float vc = ec * ec;
        r.vl = fmaxf(vu, vc);
        const float u1 = tie_weight(vu, vc);
        const float u2 = (-h.vf_clip_coef <= dv && dv <= h.vf_clip_coef) ? 1.f - u1 : 0.f;
        r.d_value = scale * (u1 * (2.f * eu) + u2 * (2.f * ec));
    } else {
        r.vl = vu;
        r.d_value = scale * (2.f * eu);
    }
    r.neg_logratio = -logratio;
    r.kl = (ratio - 1.f) - logratio;
    r.clipped = fabsf(ratio - 1.f) > h.clip_coef ? 1.f : 0.f;
    return r;
}

// the scalars of one optimiser step, from the gradient's sum of squares and the ADVANCED running products
struct StepScalars {
    float total, coef, bc1, rbc2;
};

GD_PPO_FN StepScalars step_scalars(double sum_sq, float max_norm, double pow1, double pow2) {
    StepScalars s;
    s.total = sqrtf((float)sum_sq);
    s.coef = fminf(1.f, max_norm / (s.total + 1e-6f));
    s.bc1 = (float)(1.0 - pow1);
    s.rbc2 = sqrtf((float)(1.0 - pow2));
    return s;
}

struct AdamCoefs {
    float omb1, b2, omb2, eps;
};

GD_PPO_FN AdamCoefs adam_coefs(double beta1, double beta2, float eps) {
    return AdamCoefs{(float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), eps};
}

GD_PPO_FN void adam(const AdamCoefs &c, const StepScalars &s, float lr, float g, float &p, float &m, float &v) {
    const float gc = g * s.coef;
    m = m + (gc - m) * c.omb1;
    v = v * c.b2 + c.omb2 * (gc * gc);
    const float step_size = lr / s.bc1;
    p = p - step_size * (m / (sqrtf(v) / s.rbc2 + c.eps));
}

}  // namespace ppo_rule
}  // namespace gd
