// Generalised advantage estimation of the device rollout buffer (rollout.hip k_gae_terms, k_gae_chain) as plain C++, so that
// the device and a host program (tests/gae_chain_host.cpp) run the same arithmetic against the serial loop.
//
// The rule (the reference's compute_gae, gpudrive/integrations/puffer/ppo.py:239-245, over the whole sorted batch; d, v, r are
// dones, values and rewards in sorted order, everything float32, no contraction, in this operation order):
//     adv[n-1] = 0;  last = 0
//     for t = n-2 .. 0:
//         nnt   = 1 - d[t+1]
//         delta = (r[t+1] + ((gamma * v[t+1]) * nnt)) - v[t]
//         last  = delta + (((gamma * gae_lambda) * nnt) * last)
//         adv[t] = last
// Split in two: terms() gives delta[t] and coef[t] = (gamma * gae_lambda) * nnt of every t, which depend on no other t, and
// the chain is last[t] = delta[t] + coef[t] * last[t+1].  Where coef[t] == 0 the chain is CUT: last[t+1] is multiplied by zero,
// so position t may start from last = +0 as position n-2 does.  Such a position is a HEAD; the heads split [0, n-1) into maximal
// runs that are independent chains, and run() walks one of them from its head down to the position after the next head.  For
// finite inputs this gives the serial loop's values.  Two float corner cases differ, because a cut drops the incoming last
// and the serial loop multiplies it by zero:
//   - a non-finite last arriving at a cut becomes NaN in the serial loop (0 * inf) and is dropped here;
//   - where delta is a zero at a cut, the sign of the serial loop's result follows the sign of 0 * last, here it is the sign
//     of delta + (+0).
// The translation unit that includes this must be compiled without contraction (-ffp-contract=off): a fused multiply-add in
// link() rounds once where the rule rounds twice.
#pragma once

#if defined(__HIPCC__)
#define GD_GAE_FN __host__ __device__ __forceinline__
#else
#define GD_GAE_FN inline
#endif

namespace gd {
namespace gae_chain {

// delta[t] and coef[t] from (r, v, d)[t+1] and v[t]; gl = gamma * gae_lambda, rounded to float32 once by the caller
GD_GAE_FN void terms(float gamma, float gl, float r1, float v1, float d1, float v0, float &delta, float &coef) {
    const float nnt = 1.f - d1;
    delta = (r1 + ((gamma * v1) * nnt)) - v0;
    coef = gl * nnt;
}

// one link of the chain
GD_GAE_FN float link(float delta, float coef, float last) { return delta + (coef * last); }

// whether position t of [0, n-1) starts a run
GD_GAE_FN bool is_head(float coef_t, long long t, long long n) { return t == n - 2 || coef_t == 0.f; }

// The run whose head is h (is_head(coef[h], h, n) holds; 0 <= h <= n-2): adv[h], adv[h-1], .. down to the position after the
// next head below h, or 0.  Returns the number of positions written.  The loads of the next position are issued before the
// link of this one, so a link's own operands are there when it is its turn; the walk itself still waits for the next
// position's coef before it goes on, so a long run advances at about one load latency per position.
template <class Load, class Store>
GD_GAE_FN long long run(long long h, Load load, Store store) {
    float last = 0.f, delta, coef;
    load(h, delta, coef);
    long long t = h;
    for (;;) {
        float nd = 0.f, nc = 0.f;
        const bool more = t > 0;
        if (more) load(t - 1, nd, nc);
        last = link(delta, coef, last);
        store(t, last);
        if (!more || nc == 0.f) break;
        delta = nd, coef = nc, t--;
    }
    return h - t + 1;
}

// the whole rule in the cut form, for a host program: every head's run, heads in any order (here descending)
inline void cut_form(long long n, float gamma, float gae_lambda, const float *d, const float *v, const float *r, float *delta,
                     float *coef, float *adv) {
    if (n <= 0) return;
    const float gl = gamma * gae_lambda;
    for (long long t = 0; t + 1 < n; t++) terms(gamma, gl, r[t + 1], v[t + 1], d[t + 1], v[t], delta[t], coef[t]);
    delta[n - 1] = coef[n - 1] = 0.f;
    adv[n - 1] = 0.f;
    for (long long h = n - 2; h >= 0; h--)
        if (is_head(coef[h], h, n))
            run(h, [&](long long t, float &dl, float &cf) { dl = delta[t], cf = coef[t]; }, [&](long long t, float a) { adv[t] = a; });
}

}  // namespace gae_chain
}  // namespace gd
