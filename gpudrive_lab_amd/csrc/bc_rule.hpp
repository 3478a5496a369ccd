// The mixture rule of the device BC policy forward (bc_policy.hip k_bc_head) as plain C++, so that the device and a host
// program (tests/bc_rule_host.cpp) run the same arithmetic.  It restates the reference's GMM head
// (gpudrive/integrations/il/model/networks.py GMM.get_gmm_params / forward) and gpudrive/integrations/il/loss.py gmm_loss.
//
// raw[0 .. 7C) are the head's outputs of one row: means [C][3], raw covariances [C][3], raw weights [C].  Everything is
// float32, no contraction, every sum runs serially in ASCENDING index (no tree):
//     logcov[i] = min(max(raw[3C + i], clip_value), 3.58352)          (torch.clamp)
//     cov[i]    = expf(logcov[i])
//     m = max_k raw[6C + k];  e[k] = expf(raw[6C + k] - m);  S = e[0] + .. + e[C-1];  weight[k] = e[k] / S
//     deterministic:  c = the first k with weight[k] == max weight;  action = mean[c]
//     sampled, given one uniform u in [0, 1) and three standard normals z:
//                     c = the first k whose running sum weight[0] + .. + weight[k] exceeds u; C - 1 if none does
//                     action[d] = mean[c][d] + sqrtf(cov[c][d]) * z[d]
//     nll of an expert action a (the detached per-row value of gmm_loss), in closed form:
//         lp[k] = ((-0.5 * sum_d (a[d] - mean[k][d])^2 / cov[k][d]) - 0.5 * sum_d logcov[k][d]) - 1.5 * log(2 pi)
//         wl[k] = lp[k] + logf(weight[k] + 1e-8);  M = max_k wl[k];  nll = -(M + logf(sum_k expf(wl[k] - M)))
// The draw is this project's: the reference draws the component with dist.Categorical and the action with
// MultivariateNormal.sample from torch's generator, whose stream cannot be reproduced, so the draw is a function of u and z.
// expf, logf and sqrtf's neighbours are the platform's (OCML on the device, libm on the host): they may differ in the last
// place.  raw is finite; C >= 1.  The translation unit that includes this must be compiled without contraction.
#pragma once

#include <math.h>

#if defined(__HIPCC__)
#define GD_BC_FN __host__ __device__ __forceinline__
#else
#define GD_BC_FN inline
#endif

namespace gd {
namespace bc_rule {

constexpr float COV_MAX = 3.58352f;
constexpr float LOG_2PI_15 = 2.756815599614018f;  // 1.5 * log(2 pi)
constexpr int ACTION_DIM = 3;
constexpr int MAX_COMPONENTS = 16;

template <class Load>
GD_BC_FN float logcov(int C, Load raw, float clip, int i) {
    const float v = raw(ACTION_DIM * C + i);
    return fminf(fmaxf(v, clip), COV_MAX);
}

struct Weights {
    float m, S;
};

template <class Load>
GD_BC_FN Weights weight_stats(int C, Load raw) {
    Weights w;
    w.m = raw(2 * ACTION_DIM * C);
    for (int k = 1; k < C; k++) w.m = fmaxf(w.m, raw(2 * ACTION_DIM * C + k));
    w.S = 0.f;
    for (int k = 0; k < C; k++) w.S = w.S + expf(raw(2 * ACTION_DIM * C + k) - w.m);
    return w;
}

template <class Load>
GD_BC_FN float weight(int C, Load raw, const Weights &w, int k) {
    return expf(raw(2 * ACTION_DIM * C + k) - w.m) / w.S;
}

// the first index of the largest weight
template <class Load>
GD_BC_FN int mode(int C, Load raw, const Weights &w) {
    int c = 0;
    float best = weight(C, raw, w, 0);
    for (int k = 1; k < C; k++) {
        const float v = weight(C, raw, w, k);
        if (v > best) best = v, c = k;
    }
    return c;
}

// the first k whose running weight sum exceeds u; the last component if none does
template <class Load>
GD_BC_FN int pick(int C, Load raw, const Weights &w, float u) {
    float run = 0.f;
    for (int k = 0; k < C; k++) {
        run = run + weight(C, raw, w, k);
        if (run > u) return k;
    }
    return C - 1;
}

template <class Load>
GD_BC_FN float sampled(int C, Load raw, float clip, int c, int d, float z) {
    return raw(ACTION_DIM * c + d) + sqrtf(expf(logcov(C, raw, clip, ACTION_DIM * c + d))) * z;
}

template <class Load>
GD_BC_FN float component_logprob(int C, Load raw, float clip, const Weights &w, const float *a, int k) {
    float q = 0.f, ls = 0.f;
    for (int d = 0; d < ACTION_DIM; d++) {
        const float lc = logcov(C, raw, clip, ACTION_DIM * k + d);
        const float diff = a[d] - raw(ACTION_DIM * k + d);
        q = q + (diff * diff) / expf(lc);
        ls = ls + lc;
    }
    const float lp = ((-0.5f * q) - 0.5f * ls) - LOG_2PI_15;
    return lp + logf(weight(C, raw, w, k) + 1e-8f);
}

template <class Load>
GD_BC_FN float nll(int C, Load raw, float clip, const Weights &w, const float *a) {
    float M = component_logprob(C, raw, clip, w, a, 0);
    for (int k = 1; k < C; k++) M = fmaxf(M, component_logprob(C, raw, clip, w, a, k));
    float s = 0.f;
    for (int k = 0; k < C; k++) s = s + expf(component_logprob(C, raw, clip, w, a, k) - M);
    return -(M + logf(s));
}

}  // namespace bc_rule
}  // namespace gd
