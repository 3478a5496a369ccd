// Host program of the device policy backward's head gradient rule (gpudrive_lab_amd/csrc/policy_grad_rule.hpp), built with g++
// by tests/policy_grad_reference.py.  policy_grad_rule_host IN OUT: IN holds int32 n, na, then logits [n][na] float32, actions
// [n] int32, d_logprob [n] and d_entropy [n] float32; OUT receives dlogits [n][na] float32.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../gpudrive_lab_amd/csrc/policy_grad_rule.hpp"

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    int32_t head[2];
    if (std::fread(head, 4, 2, f) != 2 || head[0] < 1 || head[1] < 1) return 4;
    const size_t n = head[0], na = head[1];
    std::vector<float> logits(n * na), dlp(n), dent(n), out(n * na);
    std::vector<int32_t> actions(n);
    if (std::fread(logits.data(), 4, n * na, f) != n * na || std::fread(actions.data(), 4, n, f) != n ||
        std::fread(dlp.data(), 4, n, f) != n || std::fread(dent.data(), 4, n, f) != n)
        return 4;
    std::fclose(f);
    for (size_t i = 0; i < n; i++) {
        const float *l = logits.data() + i * na;
        const gd::policy_grad_rule::Stats s = gd::policy_grad_rule::stats((int)na, [&](int k) { return l[k]; });
        for (size_t k = 0; k < na; k++)
            out[i * na + k] = gd::policy_grad_rule::dlogit(l[k], (int32_t)k == actions[i], s, dlp[i], dent[i]);
    }
    f = std::fopen(argv[2], "wb");
    if (!f) return 5;
    std::fwrite(out.data(), 4, n * na, f);
    return std::fclose(f) == 0 ? 0 : 5;
}
