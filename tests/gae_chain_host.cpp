// Runs csrc/gae_chain.hpp on the host: the cut form (terms, heads, one run per head -- what rollout.hip's kernels execute) and,
// beside it, the serial loop of the rule (tests/gae_serial.h).  stdin: int32 n, float gamma, float gae_lambda, then d[n], v[n],
// r[n] as float32; stdout: adv[n] of the cut form, then adv[n] of the serial loop.  Build with -ffp-contract=off.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../gpudrive_lab_amd/csrc/gae_chain.hpp"
#include "gae_serial.h"

int main() {
    int32_t n;
    float gamma, lam;
    if (fread(&n, 4, 1, stdin) != 1 || fread(&gamma, 4, 1, stdin) != 1 || fread(&lam, 4, 1, stdin) != 1 || n < 1) return 2;
    std::vector<float> d(n), v(n), r(n), delta(n), coef(n), cut(n), serial(n);
    for (std::vector<float> *a : {&d, &v, &r})
        if (fread(a->data(), 4, n, stdin) != (size_t)n) return 2;
    gd::gae_chain::cut_form(n, gamma, lam, d.data(), v.data(), r.data(), delta.data(), coef.data(), cut.data());
    gae_serial(n, gamma, lam, d.data(), v.data(), r.data(), serial.data());
    fwrite(cut.data(), 4, n, stdout);
    fwrite(serial.data(), 4, n, stdout);
    return 0;
}
