// The host program of gpudrive_lab_amd/csrc/bc_readout_rule.hpp: the read-out rule on plain arrays, for tests/test_bc_readout.py.
// Built with g++ -ffp-contract=off.  usage: bc_readout_rule_host in.bin out.bin
//   in:  [n, m] int32; logits [n][64] f32; w [64][64] f32 (an 'other' probe's head.weight); h [m][64] f32; labels [m] int64
//   out: class [n] u8; per intervened row ok u8 [m], then h' [m][64] f32; bad_labels int32 (the rows whose label is no class)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../gpudrive_lab_amd/csrc/bc_readout_rule.hpp"

namespace RR = gd::bc_readout_rule;

template <class T>
static std::vector<T> take(FILE *f, size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) {
        fprintf(stderr, "bc_readout_rule_host: input too short\n");
        exit(2);
    }
    return v;
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb");
    if (!in) return 2;
    const std::vector<int32_t> head = take<int32_t>(in, 2);
    const size_t n = (size_t)head[0], m = (size_t)head[1];
    const std::vector<float> logits = take<float>(in, n * 64), w = take<float>(in, 64 * 64), h = take<float>(in, m * 64);
    const std::vector<int64_t> labels = take<int64_t>(in, m);
    fclose(in);
    std::vector<unsigned char> cls(n), ok(m);
    std::vector<float> hp(m * 64);
    int32_t bad = 0;
    for (size_t i = 0; i < n; i++) {
        const float *z = logits.data() + i * 64;
        cls[i] = RR::class_of([&](int c) { return z[c]; });
    }
    for (size_t i = 0; i < m; i++) {
        const bool good = RR::label_ok(labels[i]);
        const float *row = w.data() + (size_t)RR::label_row(labels[i]) * 64;
        ok[i] = good ? 1 : 0;
        bad += good ? 0 : 1;
        for (int k = 0; k < 64; k++) hp[i * 64 + k] = RR::intervened(h[i * 64 + k], row[k], good);
    }
    FILE *out = fopen(argv[2], "wb");
    if (!out) return 2;
    fwrite(cls.data(), 1, n, out);
    fwrite(ok.data(), 1, m, out);
    fwrite(hp.data(), sizeof(float), m * 64, out);
    fwrite(&bad, sizeof(bad), 1, out);
    fclose(out);
    return 0;
}
