// The BC policy forward at network_dim = 128 (bc_policy_wide.hip): what bc_tile.hpp is to the 64-wide kernels, beside it so
// that those compile to the figures they had.  A wave keeps 32 tokens transposed as there; a lane now has FOUR 16-register
// accumulators, holding the features 32 t + acc_row(r, h) of its token for t < 4.  A 128 x 128 Linear is 256
// v_mfma_f32_32x32x2_f32 with the accumulator as the B operand (linear64's scheme with t, t2 < 4), LayerNorm a sum over a
// lane's 64 registers plus one swap of the lane halves.  The four heads have 32 channels each: head hd is exactly tile t = hd.
// The GMM head behind head.input_layer stays 64 wide (F, W64 of bc_tile.hpp); the context is 3 * 128 = 384 wide.
// gpudrive_lab_amd/bc_policy.py `pack_index(..., network_dim=128)` states the layout these offsets read.
#pragma once

#include "bc_tile.hpp"

namespace gd {

namespace {

constexpr int FW = 128, TW = FW / 32, CTXW = 3 * FW, W128 = FW * FW;
// 32^-1/2 as the float32 nearest to it (0x3e3504f3); q is multiplied once, after the bias
constexpr float QSCALE_W = 0.17677669529663687f;

// offsets inside one self-attention layer at 128, in floats: S_* of bc_tile.hpp with every field at its wide size
constexpr int WS_NG = 0, WS_NB = FW, WS_QW = 2 * FW, WS_QB = WS_QW + W128, WS_KW = WS_QB + FW, WS_KB = WS_KW + W128,
              WS_VW = WS_KB + FW, WS_VB = WS_VW + W128, WS_OW = WS_VB + FW, WS_OB = WS_OW + W128, WS_MG = WS_OB + FW,
              WS_MB = WS_MG + FW, WS_W1 = WS_MB + FW, WS_B1 = WS_W1 + W128, WS_W2 = WS_B1 + FW, WS_B2 = WS_W2 + W128,
              WS_SIZE = WS_B2 + FW;
// a cross-attention layer: q_norm, kv_norm (the body's norm slot), then the same fields
constexpr int WC_QG = 0, WC_QB = FW, WC_KVG = 2 * FW, WC_KVB = 3 * FW, WC_BODY = 2 * FW, WC_SIZE = WS_SIZE + WC_BODY;

BCLayout bc_layout_wide(int R, int n_self, int head_layers, int C) {
    BCLayout L;
    int o = 0;
    auto take = [&](int n) { const int at = o; o += n; return at; };
    const int kin[3] = {EGO_K * R, PARTNER_K * R, ROAD_K * R};
    for (int e = 0; e < 3; e++) {
        L.net_w0[e] = take(TW * first_steps(kin[e]) * 64);
        L.net_rest[e] = take(3 * FW + 3 * (W128 + 3 * FW));
    }
    L.self0 = take(n_self * WS_SIZE);
    L.cross[0] = take(WC_SIZE), L.cross[1] = take(WC_SIZE);
    L.head_in_w = take(CTXW * F), L.head_in_b = take(F);
    L.head_res = take(head_layers * (W64 + F));
    L.head_w = take(F * 7 * C), L.head_b = take(7 * C);
    L.total = o;
    return L;
}

// o = W a + b on the transposed tile; w is packed [t2 4][t 4][r 16][lane] = W[32 t2 + c][32 t + acc(r, h)]
__device__ __forceinline__ void linear128(const f16v (&a)[TW], const float *__restrict__ w, const float *__restrict__ b,
                                          f16v (&o)[TW], int lane, int h) {
#pragma unroll
    for (int t2 = 0; t2 < TW; t2++) {
#pragma unroll
        for (int r = 0; r < 16; r++) o[t2][r] = b[32 * t2 + acc_row(r, h)];
#pragma unroll
        for (int t = 0; t < TW; t++)
#pragma unroll
            for (int r = 0; r < 16; r++)
                o[t2] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[((t2 * TW + t) * 16 + r) * 64 + lane], a[t][r], o[t2], 0, 0, 0);
    }
}

// LayerNorm over the 128 features of this lane's token (64 here, 64 in the other lane half), biased variance, affine; in place
__device__ __forceinline__ void layer_norm128(f16v (&a)[TW], const float *__restrict__ g, const float *__restrict__ be, int h) {
    float sum = 0.f;
#pragma unroll
    for (int t = 0; t < TW; t++)
#pragma unroll
        for (int r = 0; r < 16; r++) sum = sum + a[t][r];
    sum = sum + __shfl_xor(sum, 32);
    const float mean = sum * (1.f / 128.f);
    float sq = 0.f;
#pragma unroll
    for (int t = 0; t < TW; t++)
#pragma unroll
        for (int r = 0; r < 16; r++) {
            a[t][r] = a[t][r] - mean;
            sq = sq + a[t][r] * a[t][r];
        }
    sq = sq + __shfl_xor(sq, 32);
    const float rstd = 1.f / sqrtf(sq * (1.f / 128.f) + LN_EPS);
#pragma unroll
    for (int t = 0; t < TW; t++)
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int f = 32 * t + acc_row(r, h);
            a[t][r] = (a[t][r] * rstd) * g[f] + be[f];
        }
}

// a token row of 128 floats (512-byte aligned) <-> the transposed tile: registers 4 q .. 4 q + 3 are 16 contiguous bytes
__device__ __forceinline__ void load_tok128(const float *__restrict__ row, f16v (&a)[TW], int h) {
#pragma unroll
    for (int t = 0; t < TW; t++)
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const f4 v = *reinterpret_cast<const f4 *>(row + 32 * t + 8 * q + 4 * h);
#pragma unroll
            for (int j = 0; j < 4; j++) a[t][4 * q + j] = v[j];
        }
}

__device__ __forceinline__ void store_tok128(float *__restrict__ row, const f16v (&a)[TW], int h) {
#pragma unroll
    for (int t = 0; t < TW; t++)
#pragma unroll
        for (int q = 0; q < 4; q++) {
            f4 v;
#pragma unroll
            for (int j = 0; j < 4; j++) v[j] = a[t][4 * q + j];
            *reinterpret_cast<f4 *>(row + 32 * t + 8 * q + 4 * h) = v;
        }
}

// the first embedder layer of a tile; w0 is packed [t 4][s ceil(K / 2)][lane] = W[32 t + c][2 s + h]
template <int KT>
__device__ __forceinline__ void embed_first128(const float *__restrict__ x, int D, int R, int base, int e,
                                               const float *__restrict__ w0, const float *__restrict__ b0, f16v (&a)[TW], int lane,
                                               int h) {
    const int kin = KT * R, ks = first_steps(kin);
#pragma unroll
    for (int t = 0; t < TW; t++)
#pragma unroll
        for (int r = 0; r < 16; r++) a[t][r] = b0[32 * t + acc_row(r, h)];
    for (int s = 0; s < ks; s++) {
        const int k = 2 * s + h;
        const float xv = k < kin ? x[(size_t)(k / KT) * D + base + e * KT + (k % KT)] : 0.f;
#pragma unroll
        for (int t = 0; t < TW; t++) a[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(w0[(t * ks + s) * 64 + lane], xv, a[t], 0, 0, 0);
    }
}

// ---- the one-token kernel: a workgroup of 128 threads, a thread per feature; buf is 128 floats of LDS.  Every thread sums
// the 128 entries itself in ascending order, so every thread holds the same bits and no sum has two owners.

__device__ __forceinline__ float block_ln128(float a, const float *__restrict__ g, const float *__restrict__ be, int tid, float *buf) {
    buf[tid] = a;
    __syncthreads();
    float sum = 0.f;
    for (int k = 0; k < FW; k++) sum = sum + buf[k];
    const float dlt = a - sum * (1.f / 128.f);
    __syncthreads();
    buf[tid] = dlt * dlt;
    __syncthreads();
    float sq = 0.f;
    for (int k = 0; k < FW; k++) sq = sq + buf[k];
    __syncthreads();
    const float rstd = 1.f / sqrtf(sq * (1.f / 128.f) + LN_EPS);
    return (dlt * rstd) * g[tid] + be[tid];
}

// out[tid] = b[tid] + sum_k wt[k][tid] v[k], ascending k; wt is the weight transposed [in 128][out 128]
__device__ __forceinline__ float block_matvec128(const float *__restrict__ wt, const float *__restrict__ b, float v, int tid, float *buf) {
    buf[tid] = v;
    __syncthreads();
    float o = b[tid];
    for (int k = 0; k < FW; k++) o = o + wt[k * FW + tid] * buf[k];
    __syncthreads();
    return o;
}

Seg self_seg_wide(int tok0, int ntok, int w) {
    Seg s{};
    s.tok0 = tok0, s.ntok = ntok, s.tiles = (ntok + 31) / 32, s.w = w;
    s.ng = w + WS_NG, s.nb = w + WS_NB, s.kw = w + WS_KW, s.kb = w + WS_KB, s.vw = w + WS_VW, s.vb = w + WS_VB;
    return s;
}

inline BCLayout bc_layout_wide(const gd_bc_policy &p) {
    return bc_layout_wide(p.num_stack, p.fusion_layers + 2 * p.branch_layers, p.head_layers, p.n_components);
}

inline Segs bc_layer_segs_wide(const gd_bc_policy &p, int layer) {
    const int A = p.max_agents;
    const BCLayout L = bc_layout_wide(p);
    Segs sg{};
    if (layer < p.fusion_layers) {
        sg.n = 1, sg.s[0] = self_seg_wide(0, A + ROADS, L.self0 + layer * WS_SIZE);
    } else {
        const int i = layer - p.fusion_layers;
        sg.n = 2;
        sg.s[0] = self_seg_wide(0, A, L.self0 + (p.fusion_layers + i) * WS_SIZE);
        sg.s[1] = self_seg_wide(A, ROADS, L.self0 + (p.fusion_layers + p.branch_layers + i) * WS_SIZE);
    }
    return sg;
}

inline Segs bc_cross_segs_wide(const gd_bc_policy &p) {
    const int A = p.max_agents;
    const BCLayout L = bc_layout_wide(p);
    Segs sg{};
    sg.n = 2;
    for (int ci = 0; ci < 2; ci++) {
        Seg &s = sg.s[ci];
        const int w = L.cross[ci], wb = w + WC_BODY;
        s.tok0 = ci ? A : 1, s.ntok = ci ? ROADS : A - 1, s.tiles = (s.ntok + 31) / 32, s.w = w;
        s.ng = w + WC_KVG, s.nb = w + WC_KVB, s.kw = wb + WS_KW, s.kb = wb + WS_KB, s.vw = wb + WS_VW, s.vb = wb + WS_VB;
    }
    return sg;
}

}  // namespace

}  // namespace gd
