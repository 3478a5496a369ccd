// The gradient of the mixture rule's nll (bc_rule.hpp) with respect to the head's raw outputs of one row, in closed form, as
// plain C++ so that the device and a host program (tests/bc_grad_rule_host.cpp) run the same arithmetic.  It follows what
// torch's autograd computes for the reference's GMM.get_gmm_params and gmm_loss (gpudrive/integrations/il/loss.py):
//
//     post[k] = expf(wl[k] - M) / sum_j expf(wl[j] - M)        the component posteriors, from the SAME wl[k] - M as the nll
//     d nll / d mean[k][d]   = -(post[k] * ((a[d] - mean[k][d]) / cov[k][d]))
//     d nll / d rawcov[k][d] = -(post[k] * ((0.5 * (a[d] - mean[k][d])^2) / cov[k][d] - 0.5))    inside the clamp
//                            = 0 exactly                                                         outside it
//         torch.clamp passes the gradient where clip_value <= raw <= 3.58352, BOTH bounds included, and nothing elsewhere
//     g[k] = post[k] * (weight[k] / (weight[k] + 1e-8))         the + 1e-8 inside the log is part of the derivative
//     d nll / d rawweight[j] = -(g[j] - weight[j] * G),  G = g[0] + .. + g[C-1]                   (the softmax's Jacobian)
//
// Everything is float32, no contraction, every sum runs serially in ASCENDING index.  Nothing is kept in an array: a value
// needed twice is computed twice, by the same expression, so a lane per output needs no scratch memory.  raw is finite;
// C >= 1.  The translation unit that includes this must be compiled without contraction.
#pragma once

#include "bc_rule.hpp"

namespace gd {
namespace bc_grad_rule {

using bc_rule::ACTION_DIM;

struct Stats {
    float M, s, G;  // max_k wl[k]; sum_k expf(wl[k] - M); sum_k g[k]
};

template <class Load>
GD_BC_FN float posterior(int C, Load raw, float clip, const bc_rule::Weights &w, const float *a, const Stats &st, int k) {
    return expf(bc_rule::component_logprob(C, raw, clip, w, a, k) - st.M) / st.s;
}

// g[k]: the posterior times d log(weight + 1e-8) / d weight times weight
template <class Load>
GD_BC_FN float weight_pull(int C, Load raw, float clip, const bc_rule::Weights &w, const float *a, const Stats &st, int k) {
    const float wk = bc_rule::weight(C, raw, w, k);
    return posterior(C, raw, clip, w, a, st, k) * (wk / (wk + 1e-8f));
}

template <class Load>
GD_BC_FN Stats stats(int C, Load raw, float clip, const bc_rule::Weights &w, const float *a) {
    Stats st;
    st.M = bc_rule::component_logprob(C, raw, clip, w, a, 0);
    for (int k = 1; k < C; k++) st.M = fmaxf(st.M, bc_rule::component_logprob(C, raw, clip, w, a, k));
    st.s = 0.f;
    for (int k = 0; k < C; k++) st.s = st.s + expf(bc_rule::component_logprob(C, raw, clip, w, a, k) - st.M);
    st.G = 0.f;
    for (int k = 0; k < C; k++) st.G = st.G + weight_pull(C, raw, clip, w, a, st, k);
    return st;
}

// torch.clamp's gradient mask: 1 on [clip, COV_MAX], bounds included
GD_BC_FN bool clamp_passes(float v, float clip) { return v >= clip && v <= bc_rule::COV_MAX; }

// d nll / d raw[i], i in [0, 7 C)
template <class Load>
GD_BC_FN float grad(int C, Load raw, float clip, const bc_rule::Weights &w, const float *a, const Stats &st, int i) {
    if (i < 2 * ACTION_DIM * C) {
        const bool mean = i < ACTION_DIM * C;
        const int e = mean ? i : i - ACTION_DIM * C, k = e / ACTION_DIM, d = e % ACTION_DIM;
        if (!mean && !clamp_passes(raw(ACTION_DIM * C + e), clip)) return 0.f;
        const float cov = expf(bc_rule::logcov(C, raw, clip, e));
        const float diff = a[d] - raw(e);
        const float post = posterior(C, raw, clip, w, a, st, k);
        if (mean) return -(post * (diff / cov));
        return -(post * ((0.5f * (diff * diff)) / cov - 0.5f));
    }
    const int j = i - 2 * ACTION_DIM * C;
    return -(weight_pull(C, raw, clip, w, a, st, j) - bc_rule::weight(C, raw, w, j) * st.G);
}

}  // namespace bc_grad_rule
}  // namespace gd
