// The probe read-outs inside the BC forward (gd_bc_forward_readout, gd_bc_forward_rows_readout, gd_bc_rollout_readout): the
// classes the reference's baselines/il/test/intervention.py reads per step from pairs of trained LinearProbPosition heads, taken
// from the chunk's scratch X right after the tapped self-attention layer, while X still holds that layer's output -- the
// forward goes on from there, nothing is encoded twice.  The rule is csrc/bc_readout_rule.hpp.
//   k_bc_readout   ONE launch per chunk for every probe and all three read-outs; a wave per tile of 32 rows, as in k_lp_rows.
//                  Partner tiles (only with 'other' probes): tile i of slot s is the partner columns 32 i .. 32 i + 31, the tokens
//                  1 + column (the last tile holds 31 rows: A - 1 is 63 or 127).  Ego tiles: token 0 of 32 consecutive slots.
//                  Per probe bc_tile.hpp's linear on the probe's packed weights -- k_lp_rows' logits, bit for bit -- the tile of
//                  logits through LDS so that a lane owns a row, lp_rule.hpp's first maximum, one byte stored per row.  The
//                  intervention adds row `label` of the paired 'other' probe's natural-layout head.weight to the ego token, one
//                  float32 add per feature, before the 'ego' probe's linear.  The first ego tile also counts the chunk's rows
//                  whose label is outside [0, 63] and adds them to bad_labels: the chunks of a stream run one after the other, so
//                  the counter has one writer at a time and needs no atomic.
// The list instantiation (List = BCRows) is keyed as the forward's: X by slot, labels and every output by the row.  `dead`
// (the closed loop without the list) drops a row whose byte is set: it is neither stored nor counted.
// No atomics, no host synchronisation, no allocation; equal inputs give equal bits.
#include "bc_tile.hpp"
#include "bc_readout_rule.hpp"

namespace gd {

namespace {

namespace RR = bc_readout_rule;
constexpr int LDW = F + 1;  // a [32 rows][64] tile in LDS, padded against bank conflicts

struct ROArgs {
    int A, L, slots, r0;  // r0: the chunk's first row in the call (the full forward: row = r0 + slot)
    int n_other, n_ego, intervene;
    const float *opacked[RR::MAX_PROBES], *oweight[RR::MAX_PROBES], *epacked[RR::MAX_PROBES];
    const int64_t *labels;
    long long label;
    unsigned char *other_pred, *ego_pred, *prime;
    long long os, es, ps;  // bytes between the rows of the three outputs
    int32_t *bad;
    const unsigned char *dead;
};

__device__ __forceinline__ int ro_sample(const ROArgs &a, int slot) { return a.r0 + slot; }
__device__ __forceinline__ int ro_sample(const ROArgs &, int slot, const BCRows &lr) { return bc_sample(slot, lr); }

// the class of this lane's row of the tile x under the probe `packed`; both lanes of a row get the same value
__device__ __forceinline__ unsigned char tile_class(const f16v (&x)[2], const float *__restrict__ packed, float *ldZ, int lane, int h,
                                                    int col) {
    f16v z[2];
    linear(x, packed, packed + W64, z, lane, h);
    __syncthreads();  // the tile before this one has been read
#pragma unroll
    for (int t = 0; t < 2; t++)
#pragma unroll
        for (int r = 0; r < 16; r++) ldZ[col * LDW + 32 * t + acc_row(r, h)] = z[t][r];
    __syncthreads();
    const float *__restrict__ zr = ldZ + col * LDW;
    return RR::class_of([&](int c) { return zr[c]; });
}

// grid (slots * ceil((A - 1) / 32) partner tiles if there is an 'other' probe, then ceil(slots / 32) ego tiles if there is an
// 'ego' probe), one wave each.  List = (BCRows): the forward on a row list
template <class... List>
__global__ __launch_bounds__(64) void k_bc_readout(ROArgs a, const float *__restrict__ X, List... lr) {
    __shared__ float ldZ[32 * LDW];
    const int lane = threadIdx.x, h = lane >> 5, col = lane & 31;
    const int tps = (a.A - 1 + 31) / 32;
    const int ptiles = a.n_other ? a.slots * tps : 0;
    int tile = blockIdx.x;
    f16v x[2];
    if (tile < ptiles) {
        const int slot = tile / tps;
        int j = (tile - slot * tps) * 32 + col;
        const bool live = j < a.A - 1;
        if (!live) j = a.A - 2;  // a lane past the end computes the last row again and stores nothing
        const int b = ro_sample(a, slot, lr...);
        if (b < 0) return;  // (workgroup-uniform, as the next one)
        if (a.dead && a.dead[b] != 0) return;
        load_tok(X + ((size_t)slot * a.L + 1 + j) * F, x, h);
        for (int q = 0; q < a.n_other; q++) {
            const unsigned char c = tile_class(x, a.opacked[q], ldZ, lane, h, col);
            if (live && h == 0) a.other_pred[(size_t)b * a.os + (size_t)q * (a.A - 1) + j] = c;
        }
        return;
    }
    tile -= ptiles;
    const int slot = tile * 32 + col;
    bool live = slot < a.slots;
    const int sl = live ? slot : a.slots - 1;
    int b = ro_sample(a, sl, lr...);
    if (b < 0) live = false, b = 0;
    if (live && a.dead && a.dead[b] != 0) live = false;
    load_tok(X + (size_t)sl * a.L * F, x, h);
    for (int q = 0; q < a.n_ego; q++) {
        const unsigned char c = tile_class(x, a.epacked[q], ldZ, lane, h, col);
        if (live && h == 0) a.ego_pred[(size_t)b * a.es + q] = c;
    }
    if (!a.intervene) return;
    const long long label = live ? (a.labels ? (long long)a.labels[b] : a.label) : 0;
    const bool ok = live && RR::label_ok(label);
    const int row = RR::label_row(ok ? label : 0);
    f16v xi[2];
    for (int p = 0; p < a.n_ego; p++) {
        const float *__restrict__ w = a.oweight[p] + (size_t)row * F;
#pragma unroll
        for (int t = 0; t < 2; t++)
#pragma unroll
            for (int r = 0; r < 16; r++) xi[t][r] = RR::intervened(x[t][r], w[32 * t + acc_row(r, h)], ok);
        const unsigned char c = tile_class(xi, a.epacked[p], ldZ, lane, h, col);
        if (live && h == 0) a.prime[(size_t)b * a.ps + p] = c;
    }
    if (tile != 0) return;
    // the chunk's rows that are read and whose label is no class: lane i takes the slots i, i + 64, ..
    int bad = 0;
    for (int s = lane; s < a.slots; s += 64) {
        const int bb = ro_sample(a, s, lr...);
        if (bb < 0 || (a.dead && a.dead[bb] != 0)) continue;
        bad += RR::label_ok(a.labels ? (long long)a.labels[bb] : a.label) ? 0 : 1;
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) bad += __shfl_xor(bad, d);
    if (lane == 0 && bad != 0) a.bad[0] = a.bad[0] + bad;
}

}  // namespace

// the self layer (of the forward's fusion_layers + branch_layers launches) after which X holds the tapped tokens
int bc_tap_layer(const gd_bc_policy &p, int tap, int layer) { return (tap == GD_LP_TAP_RO ? p.fusion_layers : 0) + layer; }

// One launch on the chunk whose scratch is X.  rows == nullptr: the full forward's chunk of `slots` rows from row r0.  Otherwise the
// list's chunk of `slots` positions from position r0 (n: the call's rows).  out-pointers of `ro` are the WHOLE call's.
void launch_bc_readout(const gd_bc_policy &p, hipStream_t st, const gd_bc_readout &ro, const unsigned char *dead, int r0, int slots,
                       const float *X, const int32_t *rows, const int32_t *count, int n) {
    ROArgs a{};
    a.A = p.max_agents, a.L = p.max_agents + ROADS, a.slots = slots, a.r0 = r0;
    a.n_other = ro.n_other, a.n_ego = ro.n_ego, a.intervene = ro.intervene;
    for (int i = 0; i < ro.n_other; i++) a.opacked[i] = ro.other[i].packed, a.oweight[i] = ro.other[i].weight;
    for (int i = 0; i < ro.n_ego; i++) a.epacked[i] = ro.ego[i].packed;
    a.labels = ro.labels, a.label = ro.label;
    a.other_pred = ro.other_pred, a.ego_pred = ro.ego_pred, a.prime = ro.ego_pred_prime;
    a.os = ro.other_stride, a.es = ro.ego_stride, a.ps = ro.prime_stride;
    a.bad = ro.bad_labels, a.dead = dead;
    const int tps = (a.A - 1 + 31) / 32;
    const unsigned tiles = (unsigned)((ro.n_other ? slots * tps : 0) + (ro.n_ego ? (slots + 31) / 32 : 0));
    if (rows) {
        const BCRows lr{rows, count, r0, n};
        hipLaunchKernelGGL(k_bc_readout<BCRows>, dim3(tiles), dim3(64), 0, st, a, X, lr);
    } else {
        hipLaunchKernelGGL(k_bc_readout<>, dim3(tiles), dim3(64), 0, st, a, X);
    }
}

}  // namespace gd
