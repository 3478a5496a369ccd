// What the device BC policy forward (bc_policy.hip) and backward (bc_grad.hip) share: the layout of gd_bc_policy.blob, the
// transposed 32-token tile (lane (c = lane & 31, h = lane >> 5) belongs to token c; its T 16-register accumulators hold the
// features 32 t + acc_row(r, h)), the Linear and the LayerNorm on it, the one-token helpers of the head kernels, and the
// segments a self-attention launch covers.  Everything has internal linkage: each translation unit compiles its own.
// The encoder's width is a parameter, T = network_dim / 32 tiles per token: 2 (network_dim 64, every kernel) or 4 (128, the
// forward and the backward).  The tile helpers deduce T from the accumulator array; the widths and the offsets of a layer's fields are
// BCEnc<T>; the layout and the segments are templates on T.  A file that exists at 64 only names BCEnc<2> once.  At T = 2
// everything here compiles to the code it was before there was a T (tools/isa_same.py is how that is checked).
#pragma once

#include <float.h>
#include <hip/hip_runtime.h>

#include <algorithm>

#include "bc_rule.hpp"
#include "engine.hpp"

namespace gd {

namespace {

typedef float f16v __attribute__((ext_vector_type(16)));
typedef float f4 __attribute__((ext_vector_type(4)));

// F is the width of the GMM head behind head.input_layer: 64 at either network_dim
constexpr int F = 64, ROADS = 200, ROAD_K = 13, PARTNER_K = 6, EGO_K = 6, W64 = F * F;
constexpr float LN_EPS = 1e-5f;
constexpr int MAX_HEAD_OUT = 7 * bc_rule::MAX_COMPONENTS;

// the encoder at network_dim = 32 T (gpudrive_lab_amd/bc_policy.py `pack_index` states the same order with the same T)
template <int T>
struct BCEnc {
    // features of a token, floats of a square weight, the context's width, channels of one of the four heads
    static constexpr int FE = 32 * T, W = FE * FE, CTX = 3 * FE, HC = FE / 4;
    // HC^-1/2, by which q is multiplied once, after the bias: 1/4, and 32^-1/2 as the float32 nearest to it (0x3e3504f3)
    static constexpr float QSCALE = T == 2 ? 0.25f : 0.17677669529663687f;
    // offsets inside one self-attention layer, in floats
    static constexpr int S_NG = 0, S_NB = FE, S_QW = 2 * FE, S_QB = S_QW + W, S_KW = S_QB + FE, S_KB = S_KW + W, S_VW = S_KB + FE,
                         S_VB = S_VW + W, S_OW = S_VB + FE, S_OB = S_OW + W, S_MG = S_OB + FE, S_MB = S_MG + FE, S_W1 = S_MB + FE,
                         S_B1 = S_W1 + W, S_W2 = S_B1 + FE, S_B2 = S_W2 + W, S_SIZE = S_B2 + FE;
    // a cross-attention layer: q_norm, kv_norm, then the same fields (q, o and the MLP transposed [in][out], k and v packed)
    static constexpr int C_QG = 0, C_QB = FE, C_KVG = 2 * FE, C_KVB = 3 * FE, C_BODY = 2 * FE, C_SIZE = S_SIZE + C_BODY;
    static_assert(T == 2 || T == 4, "network_dim is 64 or 128");
};

struct BCLayout {
    int net_w0[3], net_rest[3];  // 0: ego, 1: partner, 2: road.  rest: b0, g0, be0, then 3 x (W packed, b, g, be)
    int self0, cross[2], head_in_w, head_in_b, head_res, head_w, head_b, total;
};

__host__ __device__ inline int first_steps(int k) { return (k + 1) / 2; }

template <int T>
BCLayout bc_layout(int R, int n_self, int head_layers, int C) {
    using E = BCEnc<T>;
    BCLayout L;
    int o = 0;
    auto take = [&](int n) { const int at = o; o += n; return at; };
    const int kin[3] = {EGO_K * R, PARTNER_K * R, ROAD_K * R};
    for (int e = 0; e < 3; e++) {
        L.net_w0[e] = take(T * first_steps(kin[e]) * 64);
        L.net_rest[e] = take(3 * E::FE + 3 * (E::W + 3 * E::FE));
    }
    L.self0 = take(n_self * E::S_SIZE);
    L.cross[0] = take(E::C_SIZE), L.cross[1] = take(E::C_SIZE);
    L.head_in_w = take(E::CTX * F), L.head_in_b = take(F);
    L.head_res = take(head_layers * (W64 + F));
    L.head_w = take(F * 7 * C), L.head_b = take(7 * C);
    L.total = o;
    return L;
}

// accumulator register r of lane half h holds this row of a 32 x 32 tile
__device__ __forceinline__ int acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// o = W a + b on the transposed tile; w is packed [t2 T][t T][r 16][lane] = W[32 t2 + c][32 t + acc(r, h)]
template <int T>
__device__ __forceinline__ void linear(const f16v (&a)[T], const float *__restrict__ w, const float *__restrict__ b, f16v (&o)[T],
                                       int lane, int h) {
#pragma unroll
    for (int t2 = 0; t2 < T; t2++) {
#pragma unroll
        for (int r = 0; r < 16; r++) o[t2][r] = b[32 * t2 + acc_row(r, h)];
#pragma unroll
        for (int t = 0; t < T; t++)
#pragma unroll
            for (int r = 0; r < 16; r++)
                o[t2] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[((t2 * T + t) * 16 + r) * 64 + lane], a[t][r], o[t2], 0, 0, 0);
    }
}

// LayerNorm over the 32 T features of this lane's token (half here, half in the other lane half), biased variance, affine; in place
template <int T>
__device__ __forceinline__ void layer_norm(f16v (&a)[T], const float *__restrict__ g, const float *__restrict__ be, int h) {
    float sum = 0.f;
#pragma unroll
    for (int t = 0; t < T; t++)
#pragma unroll
        for (int r = 0; r < 16; r++) sum = sum + a[t][r];
    sum = sum + __shfl_xor(sum, 32);
    const float mean = sum * (1.f / (32 * T));
    float sq = 0.f;
#pragma unroll
    for (int t = 0; t < T; t++)
#pragma unroll
        for (int r = 0; r < 16; r++) {
            a[t][r] = a[t][r] - mean;
            sq = sq + a[t][r] * a[t][r];
        }
    sq = sq + __shfl_xor(sq, 32);
    const float rstd = 1.f / sqrtf(sq * (1.f / (32 * T)) + LN_EPS);
#pragma unroll
    for (int t = 0; t < T; t++)
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int f = 32 * t + acc_row(r, h);
            a[t][r] = (a[t][r] * rstd) * g[f] + be[f];
        }
}

// a token row of 32 T floats (128 T-byte aligned) <-> the transposed tile: registers 4 q .. 4 q + 3 are 16 contiguous bytes
template <int T>
__device__ __forceinline__ void load_tok(const float *__restrict__ row, f16v (&a)[T], int h) {
#pragma unroll
    for (int t = 0; t < T; t++)
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const f4 v = *reinterpret_cast<const f4 *>(row + 32 * t + 8 * q + 4 * h);
#pragma unroll
            for (int j = 0; j < 4; j++) a[t][4 * q + j] = v[j];
        }
}

template <int T>
__device__ __forceinline__ void store_tok(float *__restrict__ row, const f16v (&a)[T], int h) {
#pragma unroll
    for (int t = 0; t < T; t++)
#pragma unroll
        for (int q = 0; q < 4; q++) {
            f4 v;
#pragma unroll
            for (int j = 0; j < 4; j++) v[j] = a[t][4 * q + j];
            *reinterpret_cast<f4 *>(row + 32 * t + 8 * q + 4 * h) = v;
        }
}

__device__ __forceinline__ float gelu_erf(float x) { return (0.5f * x) * (1.f + erff(x * 0.70710678118654752440f)); }

struct BCDims {
    int A, R, L, D;  // agents, stack, tokens per sample, floats per obs row
};

struct Seg {
    int tok0, ntok, tiles;
    int w;  // k_bc_attn: the layer's offset in the blob.  k_bc_kv: unused
    int ng, nb, kw, kb, vw, vb;  // k_bc_kv: the norm and the k / v projections, offsets in the blob
};

struct Segs {
    Seg s[2];
    int n;
};

// the mask byte of global token g of sample b: the last time index of the dataset's masks
__device__ __forceinline__ unsigned char token_mask(const BCDims &d, const unsigned char *__restrict__ pm,
                                                    const unsigned char *__restrict__ rm, int b, int g) {
    if (g == 0) return 0;
    if (g < d.A) return pm[((size_t)b * d.R + d.R - 1) * (d.A - 1) + (g - 1)];
    return rm[((size_t)b * d.R + d.R - 1) * ROADS + (g - d.A)];
}

constexpr int MAX_TOKENS = 128 + ROADS;

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) v = v + __shfl_xor(v, d);
    return v;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) v = fmaxf(v, __shfl_xor(v, d));
    return v;
}

__device__ __forceinline__ float wave_ln(float a, const float *__restrict__ g, const float *__restrict__ be, int lane) {
    const float mean = wave_sum(a) * (1.f / 64.f);
    const float dlt = a - mean;
    const float rstd = 1.f / sqrtf(wave_sum(dlt * dlt) * (1.f / 64.f) + LN_EPS);
    return (dlt * rstd) * g[lane] + be[lane];
}

// out[lane] = b[lane] + sum_k wt[k][lane] v[k], ascending k; wt is the weight transposed [in 64][out 64]
__device__ __forceinline__ float matvec64(const float *__restrict__ wt, const float *__restrict__ b, float v, int lane) {
    float o = b[lane];
    for (int k = 0; k < F; k++) o = o + wt[k * F + lane] * __shfl(v, k);
    return o;
}

// the same two for a workgroup of 128 threads, a thread per feature of a 128-wide token; buf is 128 floats of LDS.  Every thread
// sums the 128 entries itself in ascending order, so every thread holds the same bits and no sum has two owners.
__device__ __forceinline__ float block_ln128(float a, const float *__restrict__ g, const float *__restrict__ be, int tid, float *buf) {
    buf[tid] = a;
    __syncthreads();
    float sum = 0.f;
    for (int k = 0; k < 128; k++) sum = sum + buf[k];
    const float dlt = a - sum * (1.f / 128.f);
    __syncthreads();
    buf[tid] = dlt * dlt;
    __syncthreads();
    float sq = 0.f;
    for (int k = 0; k < 128; k++) sq = sq + buf[k];
    __syncthreads();
    const float rstd = 1.f / sqrtf(sq * (1.f / 128.f) + LN_EPS);
    return (dlt * rstd) * g[tid] + be[tid];
}

// out[tid] = b[tid] + sum_k wt[k][tid] v[k], ascending k; wt is the weight transposed [in 128][out 128]
__device__ __forceinline__ float block_matvec128(const float *__restrict__ wt, const float *__restrict__ b, float v, int tid, float *buf) {
    buf[tid] = v;
    __syncthreads();
    float o = b[tid];
    for (int k = 0; k < 128; k++) o = o + wt[k * 128 + tid] * buf[k];
    __syncthreads();
    return o;
}

struct BCHeadArgs {
    int head_layers, C, deterministic;
    float clip;
    const float *u, *z, *expert;
    float *context, *means, *logcov, *cov, *weights, *actions, *nll, *ego_attn_score;
    int32_t *component;
};

template <int T>
Seg self_seg(int tok0, int ntok, int w) {
    using E = BCEnc<T>;
    Seg s{};
    s.tok0 = tok0, s.ntok = ntok, s.tiles = (ntok + 31) / 32, s.w = w;
    s.ng = w + E::S_NG, s.nb = w + E::S_NB, s.kw = w + E::S_KW, s.kb = w + E::S_KB, s.vw = w + E::S_VW, s.vb = w + E::S_VB;
    return s;
}

// the first embedder layer of a tile: gathers the token's R rows from obs (time is the slow index inside a token); w0 is packed
// [t T][s ceil(K / 2)][lane] = W[32 t + c][2 s + h]
template <int KT, int T>
__device__ __forceinline__ void embed_first(const float *__restrict__ x, int D, int R, int base, int e, const float *__restrict__ w0,
                                            const float *__restrict__ b0, f16v (&a)[T], int lane, int h) {
    const int kin = KT * R, ks = first_steps(kin);
#pragma unroll
    for (int t = 0; t < T; t++)
#pragma unroll
        for (int r = 0; r < 16; r++) a[t][r] = b0[32 * t + acc_row(r, h)];
    for (int s = 0; s < ks; s++) {
        const int k = 2 * s + h;
        const float xv = k < kin ? x[(size_t)(k / KT) * D + base + e * KT + (k % KT)] : 0.f;
#pragma unroll
        for (int t = 0; t < T; t++) a[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(w0[(t * ks + s) * 64 + lane], xv, a[t], 0, 0, 0);
    }
}

template <int T>
inline BCLayout bc_layout(const gd_bc_policy &p) {
    return bc_layout<T>(p.num_stack, p.fusion_layers + 2 * p.branch_layers, p.head_layers, p.n_components);
}

inline BCDims bc_dims(const gd_bc_policy &p) {
    const int A = p.max_agents;
    return BCDims{A, p.num_stack, A + ROADS, EGO_K + PARTNER_K * (A - 1) + ROAD_K * ROADS};
}

// self-attention layer `layer` of the fusion_layers + branch_layers launches: a fusion layer over all L tokens, or ro_attn and
// rg_attn layer (layer - fusion_layers) as the two segments of one launch
template <int T>
inline Segs bc_layer_segs(const gd_bc_policy &p, int layer) {
    constexpr int S_SIZE = BCEnc<T>::S_SIZE;
    const int A = p.max_agents;
    const BCLayout L = bc_layout<T>(p);
    Segs sg{};
    if (layer < p.fusion_layers) {
        sg.n = 1, sg.s[0] = self_seg<T>(0, A + ROADS, L.self0 + layer * S_SIZE);
    } else {
        const int i = layer - p.fusion_layers;
        sg.n = 2;
        sg.s[0] = self_seg<T>(0, A, L.self0 + (p.fusion_layers + i) * S_SIZE);
        sg.s[1] = self_seg<T>(A, ROADS, L.self0 + (p.fusion_layers + p.branch_layers + i) * S_SIZE);
    }
    return sg;
}

// the two cross attentions' keys and values: the kv_norm'ed partner tokens and road tokens
template <int T>
inline Segs bc_cross_segs(const gd_bc_policy &p) {
    using E = BCEnc<T>;
    const int A = p.max_agents;
    const BCLayout L = bc_layout<T>(p);
    Segs sg{};
    sg.n = 2;
    for (int ci = 0; ci < 2; ci++) {
        Seg &s = sg.s[ci];
        const int w = L.cross[ci], wb = w + E::C_BODY;
        s.tok0 = ci ? A : 1, s.ntok = ci ? ROADS : A - 1, s.tiles = (s.ntok + 31) / 32, s.w = w;
        s.ng = w + E::C_KVG, s.nb = w + E::C_KVB, s.kw = wb + E::S_KW, s.kb = wb + E::S_KB, s.vw = wb + E::S_VW, s.vb = wb + E::S_VB;
    }
    return sg;
}

// ---- the row list

// A row list on the device and the chunk of it a launch covers: the workgroup of scratch slot s has list position q0 + s
struct BCRows {
    const int32_t *rows, *count;
    int q0, n;
};

// The sample of scratch slot `slot`.  The forward's four kernels (bc_policy.hip) and k_bc_readout (bc_readout.hip) take the list as a parameter pack that is empty in the full
// forward, whose sample is the slot itself (those instantiations are the kernels as they were before there was a list).  With a
// list: row rows[q0 + slot], or -1 where the position is past the list (a length above n is read as n) or the entry is outside
// [0, n).  Workgroup-uniform; the only loads a workgroup that returns makes.
__device__ __forceinline__ int bc_sample(int slot) { return slot; }
__device__ __forceinline__ int bc_sample(int slot, const BCRows &lr) {
    const int q = lr.q0 + slot, c = *lr.count;
    if (q >= (c < lr.n ? c : lr.n)) return -1;
    const int r = lr.rows[q];
    return r >= 0 && r < lr.n ? r : -1;
}

}  // namespace

}  // namespace gd
