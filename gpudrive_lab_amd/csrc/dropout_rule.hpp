// The dropout mask rule of the device policy (policy.hip, policy_grad.hip) as plain C++, so that the forward, the backward and
// a host program (tests/dropout_rule_host.cpp) state it once.
//
// The rule is this project's: nn.Dropout draws from torch's generator, whose stream cannot be reproduced, so whether an
// element is kept is a pure function of (seed, call, row, site, entity, feature) instead -- stateless and counter-based:
//     site     0 ego embedder (entity 0), 1 partner embedder, 2 road embedder (after the tanh of each, features 0..63),
//              3 shared_embed (after its linear, entity 0, features 0..127)
//     call     the index of the forward / evaluate call (a device counter, gd_dropout.call); row the observation row
//     o[0..4)  = Philox4x32-10(counter = (call low, call high, row, word), key = (seed low, seed high)),
//                word = site << 24 | entity << 8 | block           (entity < 256, block < 16)
//     block    = block_of(feature)  = (feature >> 4) << 1 | ((feature >> 2) & 1)
//     field    = field_of(feature)  = ((feature >> 3) & 1) << 2 | (feature & 3)                       (0..7)
//     value    = 16 bits of o: (o[field >> 1] >> 16 (field & 1)) & 0xffff
//     dropped  iff value < T,  T = floor(p * 65536) computed once on the host (gd_dropout.threshold, 1..65535)
//     kept:    x * scale, scale = 1.f / (1.f - p) in float32 (torch's arithmetic at equal masks);   dropped: +0.f
// One Philox call serves 8 features.  The feature -> (block, field) map follows the accumulator layout of the MFMA kernels:
// register r of tile t in lane half h holds feature 32 t + (r & 3) + 8 (r >> 2) + 4 h, so the registers 8 m .. 8 m + 7 of one
// (t, h) are exactly block ((2 t + m) << 1 | h), fields 0..7 in register order: a lane consumes whole calls and wastes nothing.
// The map is a bijection of 0..63 onto 8 blocks x 8 fields and of 0..127 onto 16 x 8.
// Philox4x32 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11): multipliers 0xD2511F53, 0xCD9E8D57, key
// increments 0x9E3779B9, 0xBB67AE85, 10 rounds.  Integer arithmetic only: host and device cannot disagree.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define GD_DROPOUT_FN __host__ __device__ __forceinline__
#else
#define GD_DROPOUT_FN inline
#endif

namespace gd {
namespace dropout_rule {

enum { SITE_EGO = 0, SITE_PARTNER = 1, SITE_ROAD = 2, SITE_SHARED = 3 };

struct Out {
    uint32_t o0, o1, o2, o3;
};

GD_DROPOUT_FN uint32_t mulhi(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * (uint64_t)b) >> 32); }

GD_DROPOUT_FN Out philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int round = 0; round < 10; round++) {
        const uint32_t hi0 = mulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = mulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0, c1 = lo1, c2 = hi0 ^ c3 ^ k1, c3 = lo0;
        k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
    }
    return Out{c0, c1, c2, c3};
}

GD_DROPOUT_FN int block_of(int feature) { return ((feature >> 4) << 1) | ((feature >> 2) & 1); }
GD_DROPOUT_FN int field_of(int feature) { return (((feature >> 3) & 1) << 2) | (feature & 3); }

// the 8 fields of one block
GD_DROPOUT_FN Out draw(uint64_t seed, uint64_t call, uint32_t row, uint32_t site, uint32_t entity, uint32_t block) {
    return philox4x32_10((uint32_t)call, (uint32_t)(call >> 32), row, (site << 24) | (entity << 8) | block, (uint32_t)seed,
                         (uint32_t)(seed >> 32));
}

// field is a compile-time constant in the MFMA kernels and a lane's own in the others
GD_DROPOUT_FN bool kept(const Out &o, int field, uint32_t threshold) {
    const uint32_t w = (field >> 1) == 0 ? o.o0 : (field >> 1) == 1 ? o.o1 : (field >> 1) == 2 ? o.o2 : o.o3;
    return ((w >> (16 * (field & 1))) & 0xffffu) >= threshold;
}

GD_DROPOUT_FN bool kept(uint64_t seed, uint64_t call, uint32_t row, uint32_t site, uint32_t entity, int feature,
                        uint32_t threshold) {
    return kept(draw(seed, call, row, site, entity, (uint32_t)block_of(feature)), field_of(feature), threshold);
}

GD_DROPOUT_FN float apply(float x, bool keep, float scale) { return keep ? x * scale : 0.f; }

// what the kernels take of gd_dropout (the call index is read from the device by every kernel that masks)
struct Args {
    uint64_t seed;
    uint32_t threshold;
    float scale;
};

}  // namespace dropout_rule
}  // namespace gd
