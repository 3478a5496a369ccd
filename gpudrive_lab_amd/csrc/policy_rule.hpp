// The action rule of the device policy forward (policy.hip k_policy_sample) as plain C++, so that the device and a host program
// (tests/policy_rule_host.cpp) run the same arithmetic.
//
// The rule is this project's: the reference draws with torch.multinomial (gpudrive/networks/late_fusion.py:30-66), whose random
// stream cannot be reproduced, so the draw is a function of one uniform u in [0, 1) per row instead.  l[0..n) are the row's
// logits, everything is float32, no contraction, every sum runs serially in ASCENDING k (no tree):
//     m    = max_k l[k];  amax = the first k with l[k] == m
//     p[k] = expf(l[k] - m)
//     S    = p[0] + p[1] + .. + p[n-1]
//     sampled:        a = the first k whose running sum p[0] + .. + p[k] (that same order) exceeds u * S; n-1 if none does
//     deterministic:  a = amax
//     logprob = (l[a] - m) - logf(S)
//     entropy = -(sum_k q[k] * expf(q[k])),  q[k] = (l[k] - m) - logf(S)      (the reference's entropy() on normalised logits)
// p is evaluated twice (for S and for the running sum) instead of being kept: the same operands give the same float.
// expf and logf are the platform's (OCML on the device, libm on the host): they may differ in the last place, which moves
// logprob and entropy by about an ulp and the draw only where u * S falls within an ulp of a running sum.
// Logits are finite (non-finite observations are outside the contract); n >= 1.
// The translation unit that includes this must be compiled without contraction (-ffp-contract=off).
#pragma once

#include <math.h>

#if defined(__HIPCC__)
#define GD_POLICY_FN __host__ __device__ __forceinline__
#else
#define GD_POLICY_FN inline
#endif

namespace gd {
namespace policy_rule {

struct Draw {
    long long action;
    float logprob, entropy;
};

// load(k) returns l[k]; it is called four times per k
template <class Load>
GD_POLICY_FN Draw draw(int n, Load load, float u, bool deterministic) {
    float m = load(0);
    int amax = 0;
    for (int k = 1; k < n; k++) {
        const float l = load(k);
        if (l > m) m = l, amax = k;
    }
    float S = 0.f;
    for (int k = 0; k < n; k++) S = S + expf(load(k) - m);
    int a = amax;
    if (!deterministic) {
        const float t = u * S;
        float run = 0.f;
        a = n - 1;
        for (int k = 0; k < n; k++) {
            run = run + expf(load(k) - m);
            if (run > t) {
                a = k;
                break;
            }
        }
    }
    const float logS = logf(S);
    float e = 0.f;
    for (int k = 0; k < n; k++) {
        const float q = (load(k) - m) - logS;
        e = e + (q * expf(q));
    }
    Draw d;
    d.action = a;
    d.logprob = (load(a) - m) - logS;
    d.entropy = -e;
    return d;
}

// The row statistics of the training side: m = max l, logS = logf(S) and H = the entropy, by draw()'s operations in draw()'s
// order.  The one statement of them outside draw(): evaluate() below and the backward's rule (policy_grad_rule.hpp) both call
// it, so that logprob and entropy of an evaluated action equal draw()'s bit for bit (the GPU tests compare them).  draw()
// keeps its own loops: it also needs the index of the maximum and the running sum, and its kernel stays compiled as it was.
struct RowStats {
    float m, logS, H;
};

template <class Load>
GD_POLICY_FN RowStats row_stats(int n, Load load) {
    float m = load(0);
    for (int k = 1; k < n; k++) {
        const float l = load(k);
        if (l > m) m = l;
    }
    float S = 0.f;
    for (int k = 0; k < n; k++) S = S + expf(load(k) - m);
    RowStats s;
    s.m = m;
    s.logS = logf(S);
    float e = 0.f;
    for (int k = 0; k < n; k++) {
        const float q = (load(k) - m) - s.logS;
        e = e + (q * expf(q));
    }
    s.H = -e;
    return s;
}

// The training-side rule (gd_policy_evaluate): logprob and entropy of a GIVEN action a in [0, n).  Nothing is drawn.
template <class Load>
GD_POLICY_FN Draw evaluate(int n, Load load, int a) {
    const RowStats s = row_stats(n, load);
    Draw d;
    d.action = a;
    d.logprob = (load(a) - s.m) - s.logS;
    d.entropy = s.H;
    return d;
}

}  // namespace policy_rule
}  // namespace gd
