// The gradient rule of csrc/bc_grad_rule.hpp on the host: tests/bc_grad_reference.py run_grad_rule_host feeds it float32 rows
// and the tests compare the result with float64 autograd of the mixture nll.  Compile without contraction:
// g++ -O2 -ffp-contract=off.
// in:  int32 n, C; float32 clip; raw [n][7 C]; expert [n][3]
// out: per row, float32: d nll / d raw [7 C], nll
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../gpudrive_lab_amd/csrc/bc_grad_rule.hpp"

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 3;
    int32_t hdr[2];
    float clip;
    if (fread(hdr, 4, 2, f) != 2 || fread(&clip, 4, 1, f) != 1) return 4;
    const int n = hdr[0], C = hdr[1];
    if (n < 0 || C < 1 || C > gd::bc_rule::MAX_COMPONENTS) return 5;
    std::vector<float> raw((size_t)n * 7 * C), expert((size_t)n * 3);
    if (fread(raw.data(), 4, raw.size(), f) != raw.size() || fread(expert.data(), 4, expert.size(), f) != expert.size()) return 6;
    fclose(f);
    std::vector<float> out;
    for (int i = 0; i < n; i++) {
        const float *r = raw.data() + (size_t)i * 7 * C;
        const float *a = expert.data() + (size_t)i * 3;
        auto load = [&](int k) { return r[k]; };
        namespace R = gd::bc_rule;
        namespace G = gd::bc_grad_rule;
        const R::Weights w = R::weight_stats(C, load);
        const G::Stats st = G::stats(C, load, clip, w, a);
        for (int k = 0; k < 7 * C; k++) out.push_back(G::grad(C, load, clip, w, a, st, k));
        out.push_back(R::nll(C, load, clip, w, a));
    }
    f = fopen(argv[2], "wb");
    if (!f) return 7;
    fwrite(out.data(), 4, out.size(), f);
    fclose(f);
    return 0;
}
