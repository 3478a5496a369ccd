// Device policy forward (gd_policy_forward): the reference's late-fusion actor-critic in eval mode
// (gpudrive/networks/late_fusion.py:170-210) on learner rows, float32 throughout, as three launches:
//   k_policy_embed   a wave per observation row.  Each embedder is computed TRANSPOSED on v_mfma_f32_32x32x2_f32: the 64
//                    features are the accumulator rows (two tiles of 32), 32 entities sit on the lanes.  Layer 1 takes the
//                    weights as the A operand and the entity rows as B straight from global memory (dword loads, so a row
//                    that starts at any dword phase needs no care); LayerNorm reduces over a lane's 32 registers plus one swap
//                    of the two lane halves; tanh is elementwise; the accumulator is then the B operand of the second 64 x 64
//                    layer with no lane movement: register r of tile t holds feature 32t + (r&3) + 8(r>>2) + 4(lane>>5), so
//                    k-step (t, r) contracts the features F and F + 4 and the packed A operand holds W2[.][F + 4(lane>>5)].
//                    The running max over entity tiles stays in registers; lanes past the entity count never enter it.  The
//                    second layer's bias is added after the max (x -> fl(x + b) is monotonic, so the result is the same).
//                    The ego embedding (one entity) is plain lane-per-feature arithmetic.  Writes features [N][192].
//   k_policy_tail    a wave per 32 rows: hidden^T = Ws . features^T (192 -> 128, four accumulator tiles), which is again the
//                    B operand of [actor; critic] . hidden^T, one tile of 32 outputs at a time.  Writes the logits and value.
//   k_policy_sample  a lane per row runs policy_rule.hpp on the row's logits.
// The weights come packed in lane order (gd_policy.blob; the layout is PolicyLayout below and gpudrive_lab_amd/policy.py).
// An MFMA is a chain of fmaf in k order with one rounding per product; everything else rounds every operation
// (-ffp-contract=off).  No LDS, no atomics; every byte of every output is stored on every call.
// Training-mode dropout (gd_policy_forward_dropout, gd_policy_evaluate_dropout) is the same three launches on the DROP
// instantiations of k_policy_embed and k_policy_tail, which mask the four sites by dropout_rule.hpp, and on k_policy_sample_drop /
// k_policy_evaluate_drop, which also advance the call index; without DROP the code is unchanged.
// The forward on a row list (gd_policy_forward_rows) is the same three launches on sibling kernels, k_policy_embed_rows,
// k_policy_tail_rows and k_policy_sample_rows[_drop], which share the bodies above and differ in the index arithmetic only: a
// wave (a lane column, a lane) is a POSITION of the device-resident list, reads the list's length and returns when it is past
// it, computes row rows[position], keeps the scratch by position and stores the outputs of that row alone.  A row's result
// never depends on the rows beside it, so a listed row gets the full forward's bits.
// The forward on an owned list (gd_policy_forward_owned) is again the same three launches on sibling kernels,
// k_policy_embed_owned, k_policy_tail_owned and k_policy_sample_owned: the list has a segment per policy, every segment starts
// at a multiple of 32 (multi_policy_rule.hpp), so a wave of either kernel lies in ONE segment and takes the weights of that
// segment's policy -- the blob pointers come by value, the segment index is wave-uniform and the chosen pointer stays scalar.
#include <hip/hip_runtime.h>

#include "dropout_rule.hpp"
#include "engine.hpp"
#include "multi_policy_rule.hpp"
#include "policy_rule.hpp"

namespace gd {

namespace {

namespace DR = dropout_rule;
namespace MP = multi_policy_rule;

// DROP: the training-mode mask of one call (dropout_rule.hpp); `call` is the value of gd_dropout.call the kernel read
struct DropCall {
    DR::Args a;
    uint64_t call;
    uint32_t row;
};

typedef float f16v __attribute__((ext_vector_type(16)));
typedef float f4 __attribute__((ext_vector_type(4)));

constexpr int F = 64, HID = 128, FEAT = 192, ROADS = 200, ROAD_K = 13, PARTNER_K = 6;
constexpr float LN_EPS = 1e-5f;

// offsets into the blob, in floats
struct PolicyLayout {
    int ego_w1, ego_b1, ego_g, ego_b, ego_w2t, ego_b2;
    int emb_w1[2], emb_b1[2], emb_g[2], emb_b[2], emb_w2[2], emb_b2[2];  // 0: partner, 1: road
    int sh_w, sh_b, ac_w, ac_b, tiles, total;
};

PolicyLayout policy_layout(int ego_width, int n_actions) {
    PolicyLayout L;
    int o = 0;
    auto take = [&](int n) { const int at = o; o += n; return at; };
    L.ego_w1 = take(F * ego_width), L.ego_b1 = take(F), L.ego_g = take(F), L.ego_b = take(F), L.ego_w2t = take(F * F), L.ego_b2 = take(F);
    for (int e = 0; e < 2; e++) {
        L.emb_w1[e] = take(2 * (e ? 7 : 3) * 64), L.emb_b1[e] = take(F), L.emb_g[e] = take(F), L.emb_b[e] = take(F);
        L.emb_w2[e] = take(2 * 32 * 64), L.emb_b2[e] = take(F);
    }
    L.tiles = (n_actions + 1 + 31) / 32;
    L.sh_w = take(4 * 96 * 64), L.sh_b = take(HID), L.ac_w = take(L.tiles * 64 * 64), L.ac_b = take(L.tiles * 32);
    L.total = o;
    return L;
}

// accumulator register r of lane half h holds this row of a 32 x 32 tile
__device__ __forceinline__ int acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// One embedder over `count` entity rows of K floats at x (K = 6: KS = 3 k-steps; K = 13: KS = 7, the 14th column is zero in
// both operands): the pooled 64 features, bias included, to out[0..64).
// REC (gd_policy_evaluate) also records the winner of every feature to win[0..64): the LOWEST entity index among the entities
// whose float32 output equals the pooled maximum.  A lane keeps, per accumulator register, the first entity tile (0..6) that
// raised its running max -- 3 bits, 8 registers to a dword -- so the index is tile * 32 + lane; the lanes that hold the wave's
// maximum then take the minimum of their indices.  The value path is the same instructions with and without REC.
// DROP: the tanh outputs are masked before the second layer -- per (t, m) one Philox call covers the registers 8 m .. 8 m + 7 of
// a[t] (dropout_rule.hpp), four calls per lane and entity tile; winners are then recorded on the masked outputs.
template <int K, int KS, bool REC, bool DROP>
__device__ __forceinline__ void embed_pool(const float *__restrict__ x, int count, const float *__restrict__ w1a,
                                           const float *__restrict__ b1, const float *__restrict__ g, const float *__restrict__ be,
                                           const float *__restrict__ w2a, const float *__restrict__ b2, float *__restrict__ out,
                                           unsigned char *__restrict__ win, int lane, const DropCall &dc, uint32_t site) {
    const int h = lane >> 5, col = lane & 31;
    float w1[2][KS], w2[2][32];
#pragma unroll
    for (int t = 0; t < 2; t++) {
#pragma unroll
        for (int s = 0; s < KS; s++) w1[t][s] = w1a[(t * KS + s) * 64 + lane];
#pragma unroll
        for (int q = 0; q < 32; q++) w2[t][q] = w2a[(t * 32 + q) * 64 + lane];
    }
    f16v best[2];
#pragma unroll
    for (int t = 0; t < 2; t++)
#pragma unroll
        for (int r = 0; r < 16; r++) best[t][r] = -INFINITY;
    unsigned first[2][2] = {{0u, 0u}, {0u, 0u}};  // REC: [t][r >> 3], 3 bits per register

    for (int base = 0; base < count; base += 32) {
        const int e = base + col;
        const bool live = e < count;
        float xs[KS];
#pragma unroll
        for (int s = 0; s < KS; s++) xs[s] = (live && KS * h + s < K) ? x[(size_t)e * K + KS * h + s] : 0.f;
        f16v a[2];
#pragma unroll
        for (int t = 0; t < 2; t++) {
#pragma unroll
            for (int r = 0; r < 16; r++) a[t][r] = b1[32 * t + acc_row(r, h)];
#pragma unroll
            for (int s = 0; s < KS; s++) a[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(w1[t][s], xs[s], a[t], 0, 0, 0);
        }
        // LayerNorm over the 64 features of this lane's entity: 32 here, 32 in the other lane half
        float sum = 0.f;
#pragma unroll
        for (int t = 0; t < 2; t++)
#pragma unroll
            for (int r = 0; r < 16; r++) sum = sum + a[t][r];
        sum = sum + __shfl_xor(sum, 32);
        const float mean = sum * (1.f / 64.f);
        float sq = 0.f;
#pragma unroll
        for (int t = 0; t < 2; t++)
#pragma unroll
            for (int r = 0; r < 16; r++) {
                a[t][r] = a[t][r] - mean;
                sq = sq + a[t][r] * a[t][r];
            }
        sq = sq + __shfl_xor(sq, 32);
        const float rstd = 1.f / sqrtf(sq * (1.f / 64.f) + LN_EPS);
#pragma unroll
        for (int t = 0; t < 2; t++)
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int f = 32 * t + acc_row(r, h);
                a[t][r] = tanhf((a[t][r] * rstd) * g[f] + be[f]);
            }
        if constexpr (DROP) {
#pragma unroll
            for (int t = 0; t < 2; t++)
#pragma unroll
                for (int m = 0; m < 2; m++) {
                    const DR::Out o = DR::draw(dc.a.seed, dc.call, dc.row, site, (uint32_t)e, (uint32_t)((((t << 1) | m) << 1) | h));
#pragma unroll
                    for (int k = 0; k < 8; k++) a[t][8 * m + k] = DR::apply(a[t][8 * m + k], DR::kept(o, k, dc.a.threshold), dc.a.scale);
                }
        }
        f16v o[2];
#pragma unroll
        for (int t2 = 0; t2 < 2; t2++) {
#pragma unroll
            for (int r = 0; r < 16; r++) o[t2][r] = 0.f;
#pragma unroll
            for (int t = 0; t < 2; t++)
#pragma unroll
                for (int r = 0; r < 16; r++)
                    o[t2] = __builtin_amdgcn_mfma_f32_32x32x2f32(w2[t2][t * 16 + r], a[t][r], o[t2], 0, 0, 0);
        }
        if (live) {
            if constexpr (REC) {
                const unsigned tile = (unsigned)base >> 5;
#pragma unroll
                for (int t = 0; t < 2; t++)
#pragma unroll
                    for (int r = 0; r < 16; r++)
                        if (o[t][r] > best[t][r])
                            first[t][r >> 3] = (first[t][r >> 3] & ~(7u << (3 * (r & 7)))) | (tile << (3 * (r & 7)));
            }
#pragma unroll
            for (int t = 0; t < 2; t++)
#pragma unroll
                for (int r = 0; r < 16; r++) best[t][r] = fmaxf(best[t][r], o[t][r]);
        }
    }
#pragma unroll
    for (int t = 0; t < 2; t++)
#pragma unroll
        for (int r = 0; r < 16; r++) {
            float v = best[t][r];
#pragma unroll
            for (int d = 1; d < 32; d <<= 1) v = fmaxf(v, __shfl_xor(v, d));
            const int f = 32 * t + acc_row(r, h);
            if (col == 0) out[f] = v + b2[f];
            if constexpr (REC) {
                // every live lane's best is at most v; a lane with no live entity holds -inf and never equals it
                int idx = best[t][r] == v ? (int)(((first[t][r >> 3] >> (3 * (r & 7))) & 7u) * 32u) + col : 255;
#pragma unroll
                for (int d = 1; d < 32; d <<= 1) idx = min(idx, __shfl_xor(idx, d));
                if (col == 0) win[f] = (unsigned char)idx;
            }
        }
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) v = v + __shfl_xor(v, d);
    return v;
}

// One wave's row: observation row `row` (which is also what the dropout rule is keyed on) to features[slot] (and, REC,
// winners[slot]).  The full forward's slot is the row; the forward on a row list stores by list position.
// DROP: da and callp are the rule's values and the device word that holds the call index; without DROP they are not read
template <bool REC, bool DROP>
__device__ __forceinline__ void policy_embed_row(const gd_policy p, const PolicyLayout L, const float *__restrict__ obs,
                                                 float *__restrict__ features, unsigned char *__restrict__ winners,
                                                 const DR::Args da, const uint64_t *__restrict__ callp, int lane, int row,
                                                 int slot) {
    DropCall dc{da, 0, (uint32_t)row};
    if constexpr (DROP) dc.call = *callp;
    const int partners = p.max_agents - 1, ew = p.ego_width;
    const size_t width = (size_t)ew + (size_t)PARTNER_K * partners + (size_t)ROAD_K * ROADS;
    const float *__restrict__ x = obs + (size_t)row * width;
    const float *__restrict__ w = p.blob;
    float *__restrict__ out = features + (size_t)slot * FEAT;

    // ego: lane f is feature f
    {
        float a = w[L.ego_b1 + lane];
        for (int k = 0; k < ew; k++) a = a + w[L.ego_w1 + lane * ew + k] * x[k];
        const float mean = wave_sum(a) * (1.f / 64.f);
        const float d = a - mean;
        const float rstd = 1.f / sqrtf(wave_sum(d * d) * (1.f / 64.f) + LN_EPS);
        float t = tanhf((d * rstd) * w[L.ego_g + lane] + w[L.ego_b + lane]);
        if constexpr (DROP)
            t = DR::apply(t, DR::kept(dc.a.seed, dc.call, dc.row, DR::SITE_EGO, 0, lane, dc.a.threshold), dc.a.scale);
        float o = w[L.ego_b2 + lane];
        for (int f = 0; f < F; f++) o = o + w[L.ego_w2t + f * F + lane] * __shfl(t, f);
        out[lane] = o;
    }
    unsigned char *__restrict__ win = REC ? winners + (size_t)slot * (2 * F) : nullptr;
    embed_pool<PARTNER_K, 3, REC, DROP>(x + ew, partners, w + L.emb_w1[0], w + L.emb_b1[0], w + L.emb_g[0], w + L.emb_b[0],
                                        w + L.emb_w2[0], w + L.emb_b2[0], out + F, win, lane, dc, DR::SITE_PARTNER);
    embed_pool<ROAD_K, 7, REC, DROP>(x + ew + PARTNER_K * partners, ROADS, w + L.emb_w1[1], w + L.emb_b1[1], w + L.emb_g[1],
                                     w + L.emb_b[1], w + L.emb_w2[1], w + L.emb_b2[1], out + 2 * F, REC ? win + F : nullptr, lane, dc,
                                     DR::SITE_ROAD);
}

template <bool REC, bool DROP>
__global__ __launch_bounds__(256) void k_policy_embed(gd_policy p, PolicyLayout L, const float *__restrict__ obs,
                                                      float *__restrict__ features, unsigned char *__restrict__ winners,
                                                      DR::Args da, const uint64_t *__restrict__ callp) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= p.num_rows) return;  // wave-uniform; nothing below synchronises across waves
    policy_embed_row<REC, DROP>(p, L, obs, features, winners, da, callp, lane, row, row);
}

// The list's length as the kernels of the forward on a row list read it: never above N, the size of the list's array
__device__ __forceinline__ int list_count(const int32_t *__restrict__ count, int n) {
    const int c = *count;
    return c < n ? c : n;
}

// The embed kernel on a row list: the wave of list position q takes row rows[q] and stores features[q].  A wave past the
// list's length, or whose entry is no row, returns at once.
template <bool DROP>
__global__ __launch_bounds__(256) void k_policy_embed_rows(gd_policy p, PolicyLayout L, const float *__restrict__ obs,
                                                           float *__restrict__ features, DR::Args da,
                                                           const uint64_t *__restrict__ callp, const int32_t *__restrict__ rows,
                                                           const int32_t *__restrict__ count) {
    const int lane = threadIdx.x & 63;
    const int pos = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pos >= list_count(count, p.num_rows)) return;  // wave-uniform
    const int row = rows[pos];
    if (row < 0 || row >= p.num_rows) return;
    policy_embed_row<false, DROP>(p, L, obs, features, nullptr, da, callp, lane, row, pos);
}

// One wave's 32 rows, a row to a lane column: the features of slot `fslot`, the dropout rule keyed on `drow`, and, where
// `store`, the scratch logits to slot `lslot` and the outputs to row `orow`.  The full forward: fslot = drow = the row clamped
// to the last one, lslot = orow = the row.
// DROP: hidden is masked after the 192 -> 128 product with its bias, before the heads: eight Philox calls per lane
template <bool DROP>
__device__ __forceinline__ void policy_tail_rows(const gd_policy p, const PolicyLayout L, const float *__restrict__ features,
                                                 float *__restrict__ logits, float *__restrict__ logits_out,
                                                 float *__restrict__ value, const DR::Args da, const uint64_t *__restrict__ callp,
                                                 int lane, int fslot, int drow, bool store, int lslot, int orow) {
    const int h = lane >> 5;
    const int na = p.n_actions;
    const float *__restrict__ w = p.blob;
    // lane half h contracts the features [96h, 96h + 96): 24 aligned 16-byte loads
    const f4 *__restrict__ fp = reinterpret_cast<const f4 *>(features + (size_t)fslot * FEAT + 96 * h);
    f16v hid[4];
#pragma unroll
    for (int t = 0; t < 4; t++)
#pragma unroll
        for (int r = 0; r < 16; r++) hid[t][r] = w[L.sh_b + 32 * t + acc_row(r, h)];
    for (int c = 0; c < 24; c++) {
        const f4 v = fp[c];
#pragma unroll
        for (int j = 0; j < 4; j++)
#pragma unroll
            for (int t = 0; t < 4; t++)
                hid[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[L.sh_w + (t * 96 + 4 * c + j) * 64 + lane], v[j], hid[t], 0, 0, 0);
    }
    if constexpr (DROP) {
        const uint64_t call = *callp;
#pragma unroll
        for (int t = 0; t < 4; t++)
#pragma unroll
            for (int m = 0; m < 2; m++) {
                const DR::Out o = DR::draw(da.seed, call, (uint32_t)drow, DR::SITE_SHARED, 0, (uint32_t)((((t << 1) | m) << 1) | h));
#pragma unroll
                for (int k = 0; k < 8; k++) hid[t][8 * m + k] = DR::apply(hid[t][8 * m + k], DR::kept(o, k, da.threshold), da.scale);
            }
    }
    for (int i = 0; i < L.tiles; i++) {
        const float *__restrict__ wa = w + L.ac_w + (size_t)i * 64 * 64 + lane;
        f16v acc;
#pragma unroll
        for (int r = 0; r < 16; r++) acc[r] = 0.f;
#pragma unroll
        for (int t = 0; t < 4; t++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[(t * 16 + r) * 64], hid[t][r], acc, 0, 0, 0);
        if (store) {
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int a = 32 * i + acc_row(r, h);
                const float v = acc[r] + w[L.ac_b + a];
                if (a < na) {
                    logits[(size_t)lslot * na + a] = v;
                    if (logits_out) logits_out[(size_t)orow * na + a] = v;
                } else if (a == na) {
                    value[orow] = v;
                }
            }
        }
    }
}

template <bool DROP>
__global__ __launch_bounds__(64) void k_policy_tail(gd_policy p, PolicyLayout L, const float *__restrict__ features,
                                                    float *__restrict__ logits, float *__restrict__ logits_out,
                                                    float *__restrict__ value, DR::Args da, const uint64_t *__restrict__ callp) {
    const int lane = threadIdx.x;
    const int row = blockIdx.x * 32 + (lane & 31);
    const int n = p.num_rows;
    const int rc = row < n ? row : n - 1;  // a lane past the end computes the last row again and stores nothing
    policy_tail_rows<DROP>(p, L, features, logits, logits_out, value, da, callp, lane, rc, rc, row < n, row, row);
}

// The tail kernel on a row list: lane column c of workgroup g is list position q = 32 g + c: features[q] in, the scratch
// logits[q] and the outputs of row rows[q] out.  A position past the list's length computes the last position again and
// stores nothing, as does an entry that is no row (its features are whatever the scratch held).
template <bool DROP>
__global__ __launch_bounds__(64) void k_policy_tail_rows(gd_policy p, PolicyLayout L, const float *__restrict__ features,
                                                         float *__restrict__ logits, float *__restrict__ logits_out,
                                                         float *__restrict__ value, DR::Args da, const uint64_t *__restrict__ callp,
                                                         const int32_t *__restrict__ rows, const int32_t *__restrict__ count) {
    const int lane = threadIdx.x;
    const int pos = blockIdx.x * 32 + (lane & 31);
    const int cnt = list_count(count, p.num_rows);
    if ((int)blockIdx.x * 32 >= cnt) return;  // wave-uniform; cnt >= 1 below
    const int pc = pos < cnt ? pos : cnt - 1;
    const int row = rows[pc];
    const bool valid = row >= 0 && row < p.num_rows;
    policy_tail_rows<DROP>(p, L, features, logits, logits_out, value, da, callp, lane, pc, valid ? row : 0, pos < cnt && valid, pc,
                           valid ? row : 0);
}

// The last launch of a masked call also advances the call index: ONE lane (row 0) stores *call + 1, and for evaluate the
// index it consumed to *used.  No other lane of this launch reads either word.
__device__ __forceinline__ void advance_call(uint64_t *__restrict__ callp, uint64_t *__restrict__ used) {
    const uint64_t c = *callp;
    if (used) *used = c;
    *callp = c + 1;
}

// policy_rule.hpp on the logits l of one row: its draw u[row], its three outputs
__device__ __forceinline__ void policy_sample_row(int na, const float *__restrict__ l, const float *__restrict__ u,
                                                  int deterministic, int64_t *__restrict__ actions, float *__restrict__ logprob,
                                                  float *__restrict__ entropy, int row) {
    const policy_rule::Draw d = policy_rule::draw(na, [&](int k) { return l[k]; }, deterministic ? 0.f : u[row], deterministic != 0);
    actions[row] = d.action;
    logprob[row] = d.logprob;
    entropy[row] = d.entropy;
}

__device__ __forceinline__ void policy_sample(int n, int na, const float *__restrict__ logits, const float *__restrict__ u,
                                              int deterministic, int64_t *__restrict__ actions, float *__restrict__ logprob,
                                              float *__restrict__ entropy) {
    const int row = blockIdx.x * 64 + threadIdx.x;
    if (row >= n) return;
    policy_sample_row(na, logits + (size_t)row * na, u, deterministic, actions, logprob, entropy, row);
}

// The sample kernels on a row list: the lane of list position q reads the scratch logits[q] and writes row rows[q].  The
// masked call's advances the call index whatever the list's length: the grid is sized for N >= 1.
__device__ __forceinline__ void policy_sample_rows(int n, int na, const float *__restrict__ logits, const float *__restrict__ u,
                                                   int deterministic, int64_t *__restrict__ actions, float *__restrict__ logprob,
                                                   float *__restrict__ entropy, const int32_t *__restrict__ rows,
                                                   const int32_t *__restrict__ count) {
    const int pos = blockIdx.x * 64 + threadIdx.x;
    if (pos >= list_count(count, n)) return;
    const int row = rows[pos];
    if (row < 0 || row >= n) return;
    policy_sample_row(na, logits + (size_t)pos * na, u, deterministic, actions, logprob, entropy, row);
}

__global__ __launch_bounds__(64) void k_policy_sample_rows(int n, int na, const float *__restrict__ logits,
                                                           const float *__restrict__ u, int deterministic,
                                                           int64_t *__restrict__ actions, float *__restrict__ logprob,
                                                           float *__restrict__ entropy, const int32_t *__restrict__ rows,
                                                           const int32_t *__restrict__ count) {
    policy_sample_rows(n, na, logits, u, deterministic, actions, logprob, entropy, rows, count);
}

__global__ __launch_bounds__(64) void k_policy_sample_rows_drop(int n, int na, const float *__restrict__ logits,
                                                                const float *__restrict__ u, int deterministic,
                                                                int64_t *__restrict__ actions, float *__restrict__ logprob,
                                                                float *__restrict__ entropy, uint64_t *__restrict__ callp,
                                                                const int32_t *__restrict__ rows,
                                                                const int32_t *__restrict__ count) {
    if (blockIdx.x == 0 && threadIdx.x == 0) advance_call(callp, nullptr);
    policy_sample_rows(n, na, logits, u, deterministic, actions, logprob, entropy, rows, count);
}

// The owned list as the kernels of gd_policy_forward_owned take it: the policies' blobs, the segmented list and the size of its
// arrays (n + 32 P positions; features and logits are indexed by position and have as many rows)
struct OwnedList {
    const float *blob[GD_POLICY_SET_MAX];
    const int32_t *rows, *start, *count;
    int n_policies, positions;
};

// The embed kernel on an owned list: the wave of position q finds its segment, takes row rows[q] with that segment's weights
// and stores features[q].  A wave in the padding or past the last segment, or whose entry is no row, returns at once.
__global__ __launch_bounds__(256) void k_policy_embed_owned(gd_policy p, PolicyLayout L, OwnedList o, const float *__restrict__ obs,
                                                            float *__restrict__ features) {
    const int lane = threadIdx.x & 63;
    const int pos = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // (the wave's index: scalar)
    const int seg = MP::segment_of(pos, o.n_policies, o.start, o.count, o.positions);
    if (seg < 0) return;  // wave-uniform
    const int row = o.rows[pos];
    if (row < 0 || row >= p.num_rows) return;
    p.blob = o.blob[seg];
    policy_embed_row<false, false>(p, L, obs, features, nullptr, DR::Args{}, nullptr, lane, row, pos);
}

// The tail kernel on an owned list: workgroup g covers the positions 32 g .. 32 g + 31, which lie in one segment because every
// segment starts at a multiple of 32.  A workgroup past its segment's end returns; a lane past the end computes the
// segment's last position again and stores nothing, as does an entry that is no row.
__global__ __launch_bounds__(64) void k_policy_tail_owned(gd_policy p, PolicyLayout L, OwnedList o, const float *__restrict__ features,
                                                          float *__restrict__ logits, float *__restrict__ logits_out,
                                                          float *__restrict__ value) {
    const int lane = threadIdx.x;
    const int first = blockIdx.x * 32;
    const int seg = MP::segment_of(first, o.n_policies, o.start, o.count, o.positions);
    if (seg < 0) return;  // wave-uniform
    const int s = o.start[seg], c = o.count[seg];
    const int end = c < o.positions - s ? s + c : o.positions;  // (first < end: the segment holds first)
    const int pos = first + (lane & 31);
    const int pc = pos < end ? pos : end - 1;
    const int row = o.rows[pc];
    const bool valid = row >= 0 && row < p.num_rows;
    p.blob = o.blob[seg];
    policy_tail_rows<false>(p, L, features, logits, logits_out, value, DR::Args{}, nullptr, lane, pc, valid ? row : 0,
                            pos < end && valid, pc, valid ? row : 0);
}

// The sample kernel on an owned list: the lane of position q reads the scratch logits[q] and writes row rows[q]
__global__ __launch_bounds__(64) void k_policy_sample_owned(int n, int na, OwnedList o, const float *__restrict__ logits,
                                                            const float *__restrict__ u, int deterministic,
                                                            int64_t *__restrict__ actions, float *__restrict__ logprob,
                                                            float *__restrict__ entropy) {
    const int pos = blockIdx.x * 64 + threadIdx.x;
    if (MP::segment_of(pos, o.n_policies, o.start, o.count, o.positions) < 0) return;
    const int row = o.rows[pos];
    if (row < 0 || row >= n) return;
    policy_sample_row(na, logits + (size_t)pos * na, u, deterministic, actions, logprob, entropy, row);
}

__global__ __launch_bounds__(64) void k_policy_sample(int n, int na, const float *__restrict__ logits, const float *__restrict__ u,
                                                      int deterministic, int64_t *__restrict__ actions,
                                                      float *__restrict__ logprob, float *__restrict__ entropy) {
    policy_sample(n, na, logits, u, deterministic, actions, logprob, entropy);
}

__global__ __launch_bounds__(64) void k_policy_sample_drop(int n, int na, const float *__restrict__ logits,
                                                           const float *__restrict__ u, int deterministic,
                                                           int64_t *__restrict__ actions, float *__restrict__ logprob,
                                                           float *__restrict__ entropy, uint64_t *__restrict__ callp) {
    if (blockIdx.x == 0 && threadIdx.x == 0) advance_call(callp, nullptr);
    policy_sample(n, na, logits, u, deterministic, actions, logprob, entropy);
}

// gd_policy_evaluate: the action rule on GIVEN actions, a lane per row.  An action outside [0, na) is clamped (memory safety
// only; such a row's logprob is that of the clamped action).
__device__ __forceinline__ void policy_evaluate(int n, int na, const float *__restrict__ logits,
                                                const int64_t *__restrict__ actions, float *__restrict__ logprob,
                                                float *__restrict__ entropy) {
    const int row = blockIdx.x * 64 + threadIdx.x;
    if (row >= n) return;
    const float *__restrict__ l = logits + (size_t)row * na;
    const int64_t a = actions[row];
    const policy_rule::Draw d = policy_rule::evaluate(na, [&](int k) { return l[k]; }, (int)(a < 0 ? 0 : a >= na ? na - 1 : a));
    logprob[row] = d.logprob;
    entropy[row] = d.entropy;
}

__global__ __launch_bounds__(64) void k_policy_evaluate(int n, int na, const float *__restrict__ logits,
                                                        const int64_t *__restrict__ actions, float *__restrict__ logprob,
                                                        float *__restrict__ entropy) {
    policy_evaluate(n, na, logits, actions, logprob, entropy);
}

__global__ __launch_bounds__(64) void k_policy_evaluate_drop(int n, int na, const float *__restrict__ logits,
                                                             const int64_t *__restrict__ actions, float *__restrict__ logprob,
                                                             float *__restrict__ entropy, uint64_t *__restrict__ callp,
                                                             uint64_t *__restrict__ used) {
    if (blockIdx.x == 0 && threadIdx.x == 0) advance_call(callp, used);
    policy_evaluate(n, na, logits, actions, logprob, entropy);
}

DR::Args drop_args(const gd_dropout &d) { return DR::Args{d.seed, d.threshold, d.scale}; }

}  // namespace

long long policy_blob_floats(int ego_width, int n_actions) { return policy_layout(ego_width, n_actions).total; }

void launch_policy_forward(const gd_policy &p, hipStream_t st, const float *obs, const float *u, bool deterministic,
                           int64_t *actions, float *logprob, float *entropy, float *value, float *logits_out) {
    const PolicyLayout L = policy_layout(p.ego_width, p.n_actions);
    const int n = p.num_rows;
    hipLaunchKernelGGL((k_policy_embed<false, false>), dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, p, L, obs, p.features,
                       (unsigned char *)nullptr, DR::Args{}, (const uint64_t *)nullptr);
    hipLaunchKernelGGL(k_policy_tail<false>, dim3((unsigned)((n + 31) / 32)), dim3(64), 0, st, p, L, p.features, p.logits, logits_out,
                       value, DR::Args{}, (const uint64_t *)nullptr);
    hipLaunchKernelGGL(k_policy_sample, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, n, p.n_actions, p.logits, u,
                       deterministic ? 1 : 0, actions, logprob, entropy);
}

// The masked forward: the same three launches on the DROP instantiations.  d.call is advanced by the last launch (the struct
// declares it const because callers only ever read it; the device owns the word).
void launch_policy_forward(const gd_policy &p, const gd_dropout &d, hipStream_t st, const float *obs, const float *u,
                           bool deterministic, int64_t *actions, float *logprob, float *entropy, float *value, float *logits_out) {
    const PolicyLayout L = policy_layout(p.ego_width, p.n_actions);
    const int n = p.num_rows;
    const DR::Args da = drop_args(d);
    hipLaunchKernelGGL((k_policy_embed<false, true>), dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, p, L, obs, p.features,
                       (unsigned char *)nullptr, da, d.call);
    hipLaunchKernelGGL(k_policy_tail<true>, dim3((unsigned)((n + 31) / 32)), dim3(64), 0, st, p, L, p.features, p.logits, logits_out,
                       value, da, d.call);
    hipLaunchKernelGGL(k_policy_sample_drop, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, n, p.n_actions, p.logits, u,
                       deterministic ? 1 : 0, actions, logprob, entropy, const_cast<uint64_t *>(d.call));
}

// The forward on a row list (gd_policy_forward_rows): the three launches with the full forward's grids -- the host does not
// know the list's length -- on the kernels that take a list position for a row.  d: null for the unmasked forward.
void launch_policy_forward_rows(const gd_policy &p, const gd_dropout *d, hipStream_t st, const float *obs, const float *u,
                                bool deterministic, int64_t *actions, float *logprob, float *entropy, float *value,
                                float *logits_out, const int32_t *rows, const int32_t *count) {
    const PolicyLayout L = policy_layout(p.ego_width, p.n_actions);
    const int n = p.num_rows;
    const dim3 embed((unsigned)((n + 3) / 4)), tail((unsigned)((n + 31) / 32)), sample((unsigned)((n + 63) / 64));
    if (d) {
        const DR::Args da = drop_args(*d);
        hipLaunchKernelGGL(k_policy_embed_rows<true>, embed, dim3(256), 0, st, p, L, obs, p.features, da, d->call, rows, count);
        hipLaunchKernelGGL(k_policy_tail_rows<true>, tail, dim3(64), 0, st, p, L, p.features, p.logits, logits_out, value, da,
                           d->call, rows, count);
        hipLaunchKernelGGL(k_policy_sample_rows_drop, sample, dim3(64), 0, st, n, p.n_actions, p.logits, u, deterministic ? 1 : 0,
                           actions, logprob, entropy, const_cast<uint64_t *>(d->call), rows, count);
    } else {
        hipLaunchKernelGGL(k_policy_embed_rows<false>, embed, dim3(256), 0, st, p, L, obs, p.features, DR::Args{},
                           (const uint64_t *)nullptr, rows, count);
        hipLaunchKernelGGL(k_policy_tail_rows<false>, tail, dim3(64), 0, st, p, L, p.features, p.logits, logits_out, value,
                           DR::Args{}, (const uint64_t *)nullptr, rows, count);
        hipLaunchKernelGGL(k_policy_sample_rows, sample, dim3(64), 0, st, n, p.n_actions, p.logits, u, deterministic ? 1 : 0,
                           actions, logprob, entropy, rows, count);
    }
}

// The forward on an owned list (gd_policy_forward_owned): three launches whatever the number of policies, with grids sized for
// the n + 32 P positions of the list's arrays -- the host knows neither the lengths nor the starts.  Always the unmasked forward.
void launch_policy_forward_owned(const gd_policy_set &ps, hipStream_t st, const float *obs, const float *u, bool deterministic,
                                 int64_t *actions, float *logprob, float *entropy, float *value, float *logits_out,
                                 const int32_t *rows, const int32_t *start, const int32_t *count) {
    gd_policy p = ps.policy[0];
    p.features = ps.features, p.logits = ps.logits;
    const PolicyLayout L = policy_layout(p.ego_width, p.n_actions);
    OwnedList o{};
    for (int i = 0; i < ps.n_policies; i++) o.blob[i] = ps.policy[i].blob;
    o.rows = rows, o.start = start, o.count = count, o.n_policies = ps.n_policies;
    const int q = o.positions = MP::list_positions(p.num_rows, ps.n_policies);
    hipLaunchKernelGGL(k_policy_embed_owned, dim3((unsigned)((q + 3) / 4)), dim3(256), 0, st, p, L, o, obs, ps.features);
    hipLaunchKernelGGL(k_policy_tail_owned, dim3((unsigned)((q + 31) / 32)), dim3(64), 0, st, p, L, o, (const float *)ps.features,
                       ps.logits, logits_out, value);
    hipLaunchKernelGGL(k_policy_sample_owned, dim3((unsigned)((q + 63) / 64)), dim3(64), 0, st, p.num_rows, p.n_actions, o,
                       (const float *)ps.logits, u, deterministic ? 1 : 0, actions, logprob, entropy);
}

// p.features and p.logits are the caller-owned buffers of gd_policy_grad here
void launch_policy_evaluate(const gd_policy &p, hipStream_t st, const float *obs, const int64_t *actions, unsigned char *winners,
                            float *logprob, float *entropy, float *value) {
    const PolicyLayout L = policy_layout(p.ego_width, p.n_actions);
    const int n = p.num_rows;
    hipLaunchKernelGGL((k_policy_embed<true, false>), dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, p, L, obs, p.features, winners,
                       DR::Args{}, (const uint64_t *)nullptr);
    hipLaunchKernelGGL(k_policy_tail<false>, dim3((unsigned)((n + 31) / 32)), dim3(64), 0, st, p, L, p.features, p.logits,
                       (float *)nullptr, value, DR::Args{}, (const uint64_t *)nullptr);
    hipLaunchKernelGGL(k_policy_evaluate, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, n, p.n_actions, p.logits, actions,
                       logprob, entropy);
}

void launch_policy_evaluate(const gd_policy &p, const gd_dropout &d, hipStream_t st, const float *obs, const int64_t *actions,
                            unsigned char *winners, float *logprob, float *entropy, float *value) {
    const PolicyLayout L = policy_layout(p.ego_width, p.n_actions);
    const int n = p.num_rows;
    const DR::Args da = drop_args(d);
    hipLaunchKernelGGL((k_policy_embed<true, true>), dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, p, L, obs, p.features, winners,
                       da, d.call);
    hipLaunchKernelGGL(k_policy_tail<true>, dim3((unsigned)((n + 31) / 32)), dim3(64), 0, st, p, L, p.features, p.logits,
                       (float *)nullptr, value, da, d.call);
    hipLaunchKernelGGL(k_policy_evaluate_drop, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, n, p.n_actions, p.logits, actions,
                       logprob, entropy, const_cast<uint64_t *>(d.call), d.used);
}

}  // namespace gd
