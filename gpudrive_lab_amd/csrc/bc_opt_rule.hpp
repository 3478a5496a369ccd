// The rule of the device BC update (bc_opt.hip: gd_bc_train_rows, gd_bc_adamw) as plain C++, so that the device and a host
// program (tests/bc_opt_rule_host.cpp) run the same arithmetic.  It is what stands around the model's forward and backward in
// one gradient step of the reference's imitation learning (baselines/il/il.py:267-303): the mean of gmm_loss's per-row value
// and its upstream gradient, the three action errors, torch.nn.utils.clip_grad_norm_(params, 20), the reference's
// get_grad_norm and torch.optim.AdamW (single-tensor form, no amsgrad, no maximize), with every rounding fixed.
//
// ARITHMETIC.  As in ppo_rule.hpp, whose ordered_sum, step_scalars, adam_coefs and adam are used unchanged: everything per row
// and per parameter is float32 and rounds every operation (compile the including unit with -ffp-contract=off); every SUM has
// float32 terms, a float64 accumulator and one order -- element i to partial i mod 256 in ascending i, then the 256 partials
// in ascending order.
//
// ROWS.  n rows; nll [n] and action [n][3] are the forward's (the deterministic action of the weights BEFORE the step), expert
// [n][3] the batch's.
//     loss          = (float) (SUM nll[b] / (double) n)
//     dx, dy, dyaw  = (float) (SUM fabsf(action[b][d] - expert[b][d]) / (double) n),  d = 0, 1, 2
//     grad_nll[b]   = 1.f / (float) n        (what loss.mean().backward() hands the model's backward), every element stored
//
// NORMS AND CLIP.  The flat gradient g [G] is cut into T tensors; tensor t is [end[t - 1], end[t]) with end[-1] = 0.
//     s_t = SUM (g * g) over the tensor's elements, the element index of the order counted from the tensor's start
//     n_t = sqrtf((float) s_t)
//     total = sqrtf((float) S),  S = s_0 + s_1 + .. in ascending t, float64;  coef = fminf(1.f, max_norm / (total + 1e-6f))
//     best = 0.f, arg = 0;  for t ascending: if (n_t > best) best = n_t, arg = t      (get_grad_norm's strict comparison: the
//         first tensor that attains the maximum; a NaN norm is never greater)
//     max_grad_norm = coef * best  (the reference measures after clip_grad_norm_ has scaled the gradients in place)
//
// ADAMW.  step, pow1, pow2 advance as in ppo_rule.hpp (one float64 product per step); bc1, rbc2 are step_scalars'.
//     decay = (float) (1.0 - (double) lr * (double) weight_decay)
//     per parameter:  p = p * decay;  then ppo_rule::adam with gc = g * coef
// weight_decay = 0 gives decay = 1.f and p * 1.f = p, so the step is then ppo_rule's Adam bit for bit.  A non-finite gradient
// propagates as in torch.  sqrtf and the divisions are correctly rounded on both sides and nothing here is transcendental, so
// the whole rule is bit-identical between the device and the host program.  Nothing in it knows the policy's network_dim: G, T
// and end carry the layout, at 64 and at 128 (gd_bc_adamw_dim) alike.
#pragma once

#include "ppo_rule.hpp"

namespace gd {
namespace bc_opt_rule {

namespace P = ppo_rule;

constexpr int LANES = P::LANES;
enum { LOSS = 0, DX_LOSS, DY_LOSS, DYAW_LOSS, GRAD_NORM, MAX_GRAD_NORM };
constexpr int MAX_TENSORS = 288;  // 48 + 16 * (4 + 2 * 4) + 36 + 2 * (4 + 2): the largest supported model's

GD_PPO_FN float mean_of(double sum, int n) { return P::mean_of(sum, n); }
GD_PPO_FN float abs_error(float action, float expert) { return fabsf(action - expert); }
GD_PPO_FN float grad_nll_of(int n) { return 1.f / (float)n; }
GD_PPO_FN float square(float g) { return g * g; }
GD_PPO_FN float tensor_norm(double s) { return sqrtf((float)s); }

// the largest tensor norm after clipping and the first tensor that attains it
struct MaxNorm {
    float value;
    int tensor;
};

template <class Norms>
GD_PPO_FN MaxNorm max_norm_of(const Norms &norms, int num_tensors, float coef) {
    float best = 0.f;
    int arg = 0;
    for (int t = 0; t < num_tensors; t++) {
        const float n = norms[t];
        if (n > best) best = n, arg = t;
    }
    return MaxNorm{coef * best, arg};
}

GD_PPO_FN float decay_of(float lr, float weight_decay) { return (float)(1.0 - (double)lr * (double)weight_decay); }

GD_PPO_FN void adamw(const P::AdamCoefs &c, const P::StepScalars &s, float lr, float decay, float g, float &p, float &m, float &v) {
    p = p * decay;
    P::adam(c, s, lr, g, p, m, v);
}

}  // namespace bc_opt_rule
}  // namespace gd
