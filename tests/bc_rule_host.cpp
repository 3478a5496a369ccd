// The mixture rule of csrc/bc_rule.hpp on the host: tests/bc_cases.py run_rule_host feeds it float32 rows and compares the
// result with the float64 restatement (tests/bc_reference.py).  Compile without contraction: g++ -O2 -ffp-contract=off.
// in:  int32 n, C, deterministic; float32 clip; raw [n][7 C]; u [n]; z [n][3]; expert [n][3]
// out: per row, float32: logcov [3 C], cov [3 C], weights [C], component, action [3], nll
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../gpudrive_lab_amd/csrc/bc_rule.hpp"

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 3;
    int32_t hdr[3];
    float clip;
    if (fread(hdr, 4, 3, f) != 3 || fread(&clip, 4, 1, f) != 1) return 4;
    const int n = hdr[0], C = hdr[1], det = hdr[2];
    if (n < 0 || C < 1 || C > gd::bc_rule::MAX_COMPONENTS) return 5;
    std::vector<float> raw((size_t)n * 7 * C), u(n), z((size_t)n * 3), expert((size_t)n * 3);
    if (fread(raw.data(), 4, raw.size(), f) != raw.size() || fread(u.data(), 4, u.size(), f) != u.size() ||
        fread(z.data(), 4, z.size(), f) != z.size() || fread(expert.data(), 4, expert.size(), f) != expert.size())
        return 6;
    fclose(f);
    std::vector<float> out;
    for (int i = 0; i < n; i++) {
        const float *r = raw.data() + (size_t)i * 7 * C;
        auto load = [&](int k) { return r[k]; };
        namespace R = gd::bc_rule;
        const R::Weights w = R::weight_stats(C, load);
        for (int k = 0; k < 3 * C; k++) out.push_back(R::logcov(C, load, clip, k));
        for (int k = 0; k < 3 * C; k++) out.push_back(expf(R::logcov(C, load, clip, k)));
        for (int k = 0; k < C; k++) out.push_back(R::weight(C, load, w, k));
        const int c = det ? R::mode(C, load, w) : R::pick(C, load, w, u[i]);
        out.push_back((float)c);
        for (int d = 0; d < 3; d++) out.push_back(det ? r[3 * c + d] : R::sampled(C, load, clip, c, d, z[(size_t)i * 3 + d]));
        out.push_back(R::nll(C, load, clip, w, expert.data() + (size_t)i * 3));
    }
    f = fopen(argv[2], "wb");
    if (!f) return 7;
    fwrite(out.data(), 4, out.size(), f);
    fclose(f);
    return 0;
}
