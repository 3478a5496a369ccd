// Host program of the device policy's action rule (gpudrive_lab_amd/csrc/policy_rule.hpp), built with g++ by
// tests/policy_cases.py.  policy_rule_host IN OUT: IN holds int32 n, na, deterministic, then logits [n][na] and u [n] float32;
// OUT receives actions [n] int64, logprob [n] and entropy [n] float32.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../gpudrive_lab_amd/csrc/policy_rule.hpp"

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    int32_t head[3];
    if (std::fread(head, 4, 3, f) != 3 || head[0] < 1 || head[1] < 1) return 4;
    const size_t n = head[0], na = head[1];
    std::vector<float> logits(n * na), u(n), logprob(n), entropy(n);
    std::vector<int64_t> actions(n);
    if (std::fread(logits.data(), 4, n * na, f) != n * na || std::fread(u.data(), 4, n, f) != n) return 4;
    std::fclose(f);
    for (size_t i = 0; i < n; i++) {
        const float *l = logits.data() + i * na;
        const gd::policy_rule::Draw d = gd::policy_rule::draw((int)na, [&](int k) { return l[k]; }, u[i], head[2] != 0);
        actions[i] = d.action, logprob[i] = d.logprob, entropy[i] = d.entropy;
    }
    f = std::fopen(argv[2], "wb");
    if (!f) return 5;
    std::fwrite(actions.data(), 8, n, f);
    std::fwrite(logprob.data(), 4, n, f);
    std::fwrite(entropy.data(), 4, n, f);
    return std::fclose(f) == 0 ? 0 : 5;
}
