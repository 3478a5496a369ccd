// The host program of csrc/dropout_rule.hpp: the mask rule the kernels use, compiled with g++ for the tests.
//   philox c0 c1 c2 c3 k0 k1                         (hex words) -> the four output words, hex
//   map                                              -> "block field" of the features 0..127, one per line
//   mask seed call T site rows entities features out -> out: rows * entities * features bytes, 1 = kept, 0 = dropped
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../gpudrive_lab_amd/csrc/dropout_rule.hpp"

namespace DR = gd::dropout_rule;

int main(int argc, char **argv) {
    if (argc >= 2 && !strcmp(argv[1], "philox") && argc == 8) {
        uint32_t w[6];
        for (int i = 0; i < 6; i++) w[i] = (uint32_t)strtoul(argv[2 + i], nullptr, 16);
        const DR::Out o = DR::philox4x32_10(w[0], w[1], w[2], w[3], w[4], w[5]);
        printf("%08x %08x %08x %08x\n", o.o0, o.o1, o.o2, o.o3);
        return 0;
    }
    if (argc == 2 && !strcmp(argv[1], "map")) {
        for (int f = 0; f < 128; f++) printf("%d %d\n", DR::block_of(f), DR::field_of(f));
        return 0;
    }
    if (argc == 10 && !strcmp(argv[1], "mask")) {
        const uint64_t seed = strtoull(argv[2], nullptr, 10), call = strtoull(argv[3], nullptr, 10);
        const uint32_t T = (uint32_t)strtoul(argv[4], nullptr, 10), site = (uint32_t)strtoul(argv[5], nullptr, 10);
        const long rows = strtol(argv[6], nullptr, 10), entities = strtol(argv[7], nullptr, 10), features = strtol(argv[8], nullptr, 10);
        if (rows < 1 || entities < 1 || entities > 256 || features < 1 || features > 128 || site > 3) return 2;
        std::vector<unsigned char> out((size_t)rows * entities * features);
        size_t at = 0;
        for (long r = 0; r < rows; r++)
            for (long e = 0; e < entities; e++)
                for (long f = 0; f < features; f++)
                    out[at++] = DR::kept(seed, call, (uint32_t)r, site, (uint32_t)e, (int)f, T) ? 1 : 0;
        FILE *fp = fopen(argv[9], "wb");
        if (!fp || fwrite(out.data(), 1, out.size(), fp) != out.size()) return 3;
        fclose(fp);
        return 0;
    }
    fprintf(stderr, "usage: philox | map | mask (see the source)\n");
    return 1;
}
