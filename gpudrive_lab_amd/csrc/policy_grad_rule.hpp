// The head gradient rule of the device policy backward (policy_grad.hip) as plain C++, so that the device and a host program
// (tests/policy_grad_rule_host.cpp) run the same arithmetic.
//
// A row has logits l[0..n), a taken action a and two upstream gradients, d_logprob and d_entropy, of
//     logprob = q[a],   entropy = H = -sum_k p[k] q[k],   q[k] = (l[k] - m) - logf(S),   p[k] = expf(q[k])
// with m = max_k l[k] and S = sum_k expf(l[k] - m) in ascending k (policy_rule.hpp).  Since dq[j]/dl[k] = 1[j = k] - p[k] and
// dH/dl[k] = -p[k] (q[k] + H),
//     dl[k] = d_logprob * (1[k = a] - p[k]) - d_entropy * (p[k] * (q[k] + H)).
// Stats is policy_rule.hpp's RowStats (m, logf(S), H), computed by its row_stats(): the one statement of those sums that
// gd_policy_evaluate uses too; dlogit() is elementwise.  A logit so far below the maximum that expf underflows has p = 0 and q
// finite: its terms are exact zeros, never 0 * inf.  Everything is float32 and rounds every operation: compile the including
// unit with -ffp-contract=off.
#pragma once

#include <math.h>

#include "policy_rule.hpp"

#if defined(__HIPCC__)
#define GD_POLICY_GRAD_FN __host__ __device__ __forceinline__
#else
#define GD_POLICY_GRAD_FN inline
#endif

namespace gd {
namespace policy_grad_rule {

using Stats = policy_rule::RowStats;

// load(k) returns l[k]; it is called three times per k
template <class Load>
GD_POLICY_GRAD_FN Stats stats(int n, Load load) {
    return policy_rule::row_stats(n, load);
}

GD_POLICY_GRAD_FN float dlogit(float l, bool taken, Stats s, float d_logprob, float d_entropy) {
    const float q = (l - s.m) - s.logS;
    const float p = expf(q);
    return d_logprob * ((taken ? 1.f : 0.f) - p) - d_entropy * (p * (q + s.H));
}

}  // namespace policy_grad_rule
}  // namespace gd
