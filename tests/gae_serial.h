/* The serial loop of the GAE rule (csrc/gae_chain.hpp states it), in C: what the cut form is held against by
 * tests/gae_chain_host.cpp and what tools/rollout_bench.py times on the host.  Compile without contraction
 * (-ffp-contract=off). */
#ifndef GD_GAE_SERIAL_H
#define GD_GAE_SERIAL_H
static inline void gae_serial(int n, float gamma, float lam, const float *d, const float *v, const float *r, float *adv) {
    float last = 0.f;
    if (n < 1) return;
    adv[n - 1] = 0.f;
    for (int t = n - 2; t >= 0; t--) {
        const float nnt = 1.f - d[t + 1];
        const float delta = (r[t + 1] + ((gamma * v[t + 1]) * nnt)) - v[t];
        last = delta + (((gamma * lam) * nnt) * last);
        adv[t] = last;
    }
}
#endif
