// Device BC policy backward (gd_bc_backward, gd_bc_backward_dim): the gradient of sum_b grad_nll[b] nll[b] with respect to every parameter of the
// model bc_policy.hip runs, float32, following torch's autograd of the reference (gmm_loss(...).backward()).  Per chunk of
// gd_bc_policy.chunk_rows rows:
//   the forward again, by bc_policy.hip's own kernels (so nll is gd_bc_forward's bit for bit), with the input of every
//   self-attention launch copied to scratch (XS[layer]);
//   k_bcg_head    (64) a wave per row, lane per feature, plain arithmetic as k_bc_head: recomputes both cross attentions and the
//                 head keeping what the backward needs in registers and LDS, then bc_grad_rule.hpp, the head, the MLPs, the
//                 one-query attentions (dV[j] = p[j] dO, dS = p (dP - sum p dP) and 0 at a masked key, dK[j] = dS[j] q,
//                 dq = sum dS[j] K[j]), q_proj and q_norm.  Owns dX[b][token 0], dKx[b][key], dVx[b][key].
//   k_bcg_kvx     a wave per 32 key tokens of a cross attention: k_proj, v_proj and kv_norm.  Owns dX[b][tokens 1 ..].
//   then layer by layer, last to first: XS[layer] is copied to X and the layer's k_bc_kv and k_bc_attn<SAVE> run again (K, V, the
//   attention output O before o_proj, the softmax's running max m and sum l per (token, head)), and
//   k_bcg_post    a wave per 32 tokens: y = o_proj(O) + x, the MLP again, then its backward and o_proj's.  Owns dX[token] (now
//                 the residual's share) and dO[token].
//   k_bcg_dq      a wave per 32 QUERIES: q again (stored to Q), then per head the keys in tiles of 32, ascending, twice:
//                 S^T = K Q^T and dP^T = V dO^T in one accumulator each, P = exp(S - m) / l; the first walk sums
//                 D = sum_j P[j] dP[j] as the softmax's backward does (not dO . O: with one unmasked key D must BE that key's
//                 dP), the second forms dS = P (dP - D), 0 at a masked key, and dQ^T += K^T dS^T.  The scores never leave
//                 registers.  Owns Q[token], dQ[token], D[token].
//   k_bcg_dkv     a wave per 32 KEYS: per head the queries in tiles of 32, ascending: S = Q K^T and dP = dO V^T with the key on
//                 the lane, P and dS from the saved m, l and D of each query row, dV^T += dO^T P, dK^T += Q^T dS; then
//                 k_proj, v_proj and q_proj back to the normed input, the LayerNorm, plus the residual's share.  Owns dX[token].
//   k_bcg_embed   a wave per 32 tokens of one kind: the four embedder layers, last to first, each recomputed from obs.
// Every product over a token tile is v_mfma_f32_32x32x2_f32 on the transposed tile of bc_tile.hpp: dX^T = W^T dY^T is linear
// with the transposed weights (k_bcg_transpose writes them once per call), dW = dY^T X contracts the tile's 32 tokens after one
// trip of both tiles through LDS.  Weight gradients: a launch has `num_partials` workgroups of one wave; workgroup w takes the
// (row, tile) pairs w, w + num_partials, .. in ascending order and adds each pair's share to ITS slice of `partials` (natural
// layout, read and written by one fixed lane), across chunks; k_bcg_reduce adds the slices in index order.  No atomics: every
// sum has one owner and a fixed order.  An MFMA is a chain of fmaf in k order; everything else rounds every operation.
// The widths are BCEnc<T>'s (bc_tile.hpp), T = network_dim / 32: the helpers and the tile kernels are one text for 64 (T = 2)
// and 128 (T = 4), and the 64-wide instantiations are the machine code they were before there was a T (tools/isa_same.py).  At
// 128 a head is tile t = hd (32 channels, all 16 registers of both lane halves: the attention passes' products take 16
// k-steps and dQ^T, dK^T, dV^T fill all 32 rows), q and dq are scaled by BCEnc<4>::QSCALE, and k_bcg_head's place is taken by
//   k_bcg_head_block  (128) a workgroup of 128 threads per row, a thread per encoder feature, every sum across its two waves
//                 through LDS with one owner and ascending order; the 64-wide GMM head and the rule on threads 0 .. 63.
#include "bc_tile.hpp"

#include "bc_grad_rule.hpp"

namespace gd {

namespace {

// a [32 tokens][32 T] tile in LDS is padded to 32 T + 1 floats a row against bank conflicts (BCEnc<T>::FE + 1, LDW below)
constexpr int LXW = 129;                         // the first embedder layer's input tile: up to 8 * 13 = 104 columns, padded to 128
constexpr int MAX_T = 104;
constexpr float INV_SQRT_2PI = 0.3989422804014327f;

// the gradient's layout: the state dict's order, natural row-major tensors.  It is the blob's layout without the first
// embedder layers' padding, so every field after the embedders sits at its blob offset plus one constant.
template <int T>
BCLayout bc_nat_layout(int R, int n_self, int head_layers, int C) {
    constexpr int FE = BCEnc<T>::FE, W = BCEnc<T>::W;
    BCLayout L = bc_layout<T>(R, n_self, head_layers, C);
    const int kin[3] = {EGO_K * R, PARTNER_K * R, ROAD_K * R};
    int o = 0;
    for (int e = 0; e < 3; e++) {
        L.net_w0[e] = o, o += FE * kin[e];
        L.net_rest[e] = o, o += 3 * FE + 3 * (W + 3 * FE);
    }
    const int delta = o - L.self0;
    L.self0 += delta, L.cross[0] += delta, L.cross[1] += delta, L.head_in_w += delta, L.head_in_b += delta, L.head_res += delta;
    L.head_w += delta, L.head_b += delta, L.total += delta;
    return L;
}

// ---- the call's own launches

__global__ __launch_bounds__(256) void k_bcg_zero(float *__restrict__ p, size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) p[i] = 0.f;
}

__global__ __launch_bounds__(256) void k_bcg_copy(const f4 *__restrict__ src, f4 *__restrict__ dst, size_t n4) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) dst[i] = src[i];
}

__global__ __launch_bounds__(256) void k_bcg_reduce(const float *__restrict__ partials, int P, long long G, float *__restrict__ grad) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= G) return;
    float s = partials[e];
    for (int p = 1; p < P; p++) s = s + partials[(size_t)p * G + e];
    grad[e] = s;
}

// the matrices the backward multiplies from the other side: off is the blob offset; nin == 0: a 32 T x 32 T matrix in the mfma
// pack, rewritten as its transpose in the same pack; otherwise a [nin][nout] matrix rewritten as [nout][nin]
struct TList {
    int n;
    int off[MAX_T], nin[MAX_T], nout[MAX_T];
};

template <int T>
__global__ __launch_bounds__(64) void k_bcg_transpose(TList tl, const float *__restrict__ blob, float *__restrict__ WT) {
    const int lane = threadIdx.x, h = lane >> 5, c = lane & 31;
    const int off = tl.off[blockIdx.x], nin = tl.nin[blockIdx.x], nout = tl.nout[blockIdx.x];
    if (nin == 0) {
        // WT[t2][t][r][lane] = W[32 t + acc(r, h)][32 t2 + c], which the pack holds at [t][t2][r'][h'][acc(r, h)] with acc(r', h') = c
        const int rp = (c & 3) + 4 * (c >> 3), hp = (c >> 2) & 1;
        for (int t2 = 0; t2 < T; t2++)
            for (int t = 0; t < T; t++)
                for (int r = 0; r < 16; r++)
                    WT[off + ((t2 * T + t) * 16 + r) * 64 + lane] = blob[off + ((t * T + t2) * 16 + rp) * 64 + hp * 32 + acc_row(r, h)];
    } else {
        for (int i = lane; i < nin * nout; i += 64) WT[off + i] = blob[off + (i % nin) * nout + i / nin];
    }
}

// ---- the transposed tile: pieces of the backward

// o = W a on the transposed tile, no bias (with the transposed pack: the gradient with respect to a Linear's input)
template <int T>
__device__ __forceinline__ void linear64_nb(const f16v (&a)[T], const float *__restrict__ w, f16v (&o)[T], int lane) {
#pragma unroll
    for (int t2 = 0; t2 < T; t2++) {
#pragma unroll
        for (int r = 0; r < 16; r++) o[t2][r] = 0.f;
#pragma unroll
        for (int t = 0; t < T; t++)
#pragma unroll
            for (int r = 0; r < 16; r++)
                o[t2] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[((t2 * T + t) * 16 + r) * 64 + lane], a[t][r], o[t2], 0, 0, 0);
        if constexpr (T > 2) asm volatile("" ::: "memory");  // (as in accum_dw: one output tile's 64 weights at a time)
    }
}

// layer_norm of bc_tile.hpp (the same operations in the same order), keeping the normalised value and 1 / std
template <int T>
__device__ __forceinline__ void layer_norm_keep(f16v (&a)[T], f16v (&xh)[T], float &rstd, const float *__restrict__ g,
                                                const float *__restrict__ be, int h) {
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
    rstd = 1.f / sqrtf(sq * (1.f / (32 * T)) + LN_EPS);
#pragma unroll
    for (int t = 0; t < T; t++)
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int f = 32 * t + acc_row(r, h);
            xh[t][r] = a[t][r] * rstd;
            a[t][r] = xh[t][r] * g[f] + be[f];
        }
}

// d: the gradient at the LayerNorm's output on entry, at its input on return (biased variance)
template <int T>
__device__ __forceinline__ void layer_norm_back(f16v (&d)[T], const f16v (&xh)[T], float rstd, const float *__restrict__ g, int h) {
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int t = 0; t < T; t++)
#pragma unroll
        for (int r = 0; r < 16; r++) {
            d[t][r] = d[t][r] * g[32 * t + acc_row(r, h)];
            s1 = s1 + d[t][r];
            s2 = s2 + d[t][r] * xh[t][r];
        }
    s1 = s1 + __shfl_xor(s1, 32);
    s2 = s2 + __shfl_xor(s2, 32);
    const float m1 = s1 * (1.f / (32 * T)), m2 = s2 * (1.f / (32 * T));
#pragma unroll
    for (int t = 0; t < T; t++)
#pragma unroll
        for (int r = 0; r < 16; r++) d[t][r] = rstd * ((d[t][r] - m1) - xh[t][r] * m2);
}

__device__ __forceinline__ float gelu_erf_grad(float x) {
    return 0.5f * (1.f + erff(x * 0.70710678118654752440f)) + (x * INV_SQRT_2PI) * expf(-0.5f * (x * x));
}

template <int T>
__device__ __forceinline__ void zero_tile(f16v (&a)[T]) {
#pragma unroll
    for (int t = 0; t < T; t++)
#pragma unroll
        for (int r = 0; r < 16; r++) a[t][r] = 0.f;
}

// the tile to LDS as [token][feature]; a lane past the segment's end contributes zeros
template <int T>
__device__ __forceinline__ void tile_to_lds(float *__restrict__ lds, const f16v (&a)[T], int col, int h, bool live) {
    constexpr int LDW = 32 * T + 1;
#pragma unroll
    for (int t = 0; t < T; t++)
#pragma unroll
        for (int r = 0; r < 16; r++) lds[col * LDW + 32 * t + acc_row(r, h)] = live ? a[t][r] : 0.f;
}

// w[o][i] += sum over the tile's 32 tokens, ascending, of dy[token][o] x[token][i]; o < 32 T, i < kin; w is [32 T][kin] in this
// workgroup's slice.  ldy is a [32][LDW] image, lx a [32][lxw] image whose columns up to the next multiple of 32 are stored.
template <int T>
__device__ __forceinline__ void accum_dw(float *__restrict__ w, int kin, const float *__restrict__ ldy, const float *__restrict__ lx,
                                         int lxw, int lane) {
    constexpr int LDW = 32 * T + 1;
    const int h = lane >> 5, c = lane & 31;
    for (int t2 = 0; t2 < T; t2++)
        for (int tk = 0; tk * 32 < kin; tk++) {
            const int col = 32 * tk + c;
            f16v acc;
#pragma unroll
            for (int r = 0; r < 16; r++) acc[r] = col < kin ? w[(32 * t2 + acc_row(r, h)) * kin + col] : 0.f;
#pragma unroll
            for (int s = 0; s < 16; s++)
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ldy[(2 * s + h) * LDW + 32 * t2 + c], lx[(2 * s + h) * lxw + col], acc, 0, 0, 0);
            if (col < kin) {
#pragma unroll
                for (int r = 0; r < 16; r++) w[(32 * t2 + acc_row(r, h)) * kin + col] = acc[r];
            }
            // at 128 the 16 blocks of a square weight are not to be loaded ahead all at once: that is 256 registers
            if constexpr (T > 2) asm volatile("" ::: "memory");
        }
}

// v[f] += sum over the tile's 32 tokens, ascending, of the [32][LDW] image's column f; lane = f, and f - 64 at 128
template <int T>
__device__ __forceinline__ void accum_vec(float *__restrict__ v, const float *__restrict__ ld, int lane) {
    constexpr int LDW = 32 * T + 1;
#pragma unroll
    for (int f0 = 0; f0 < 32 * T; f0 += 64) {
        float s = v[f0 + lane];
        for (int tok = 0; tok < 32; tok++) s = s + ld[tok * LDW + f0 + lane];
        v[f0 + lane] = s;
    }
}

// one Linear's share of a tile: dW += dy (x) x through both LDS images, db += dy
template <int T>
__device__ __forceinline__ void linear_grads(float *__restrict__ w, float *__restrict__ b, const f16v (&dy)[T], const f16v (&x)[T],
                                             float *__restrict__ ldA, float *__restrict__ ldB, int lane, bool live) {
    const int h = lane >> 5, c = lane & 31;
    __syncthreads();
    tile_to_lds(ldA, dy, c, h, live);
    tile_to_lds(ldB, x, c, h, live);
    __syncthreads();
    accum_dw<T>(w, 32 * T, ldA, ldB, 32 * T + 1, lane);
    accum_vec<T>(b, ldA, lane);
}

// a LayerNorm's share of a tile: dgain += d xhat, dbias += d (d: the gradient at its output)
template <int T>
__device__ __forceinline__ void norm_grads(float *__restrict__ g, float *__restrict__ b, const f16v (&d)[T], const f16v (&xh)[T],
                                           float *__restrict__ ldA, float *__restrict__ ldB, int lane, bool live) {
    const int h = lane >> 5, c = lane & 31;
    f16v p[T];
#pragma unroll
    for (int t = 0; t < T; t++)
#pragma unroll
        for (int r = 0; r < 16; r++) p[t][r] = d[t][r] * xh[t][r];
    __syncthreads();
    tile_to_lds(ldA, p, c, h, live);
    tile_to_lds(ldB, d, c, h, live);
    __syncthreads();
    accum_vec<T>(g, ldA, lane);
    accum_vec<T>(b, ldB, lane);
}

// tile id -> (row, segment, tile in segment)
struct TileAt {
    int b, second, tile;
};

__device__ __forceinline__ TileAt tile_at(const Segs &sg, int id) {
    const int per = sg.s[0].tiles + (sg.n > 1 ? sg.s[1].tiles : 0);
    TileAt a;
    a.b = id / per;
    a.tile = id % per;
    a.second = a.tile >= sg.s[0].tiles;
    if (a.second) a.tile -= sg.s[0].tiles;
    return a;
}

__host__ __device__ inline int tiles_of(const Segs &sg) { return sg.s[0].tiles + (sg.n > 1 ? sg.s[1].tiles : 0); }

struct GradBufs {
    const float *blob, *WT;
    float *partials;   // [gridDim.x][G]
    long long G;
    int nat_delta;     // natural offset = blob offset + nat_delta for every field after the embedders
    float *dX, *dO, *dQ, *Q, *O, *ML, *D;  // [rows][L][64] each; ML [rows][L][8]; D [rows][L][4]
};

// ---- a self-attention layer, last part first

// grid (num_partials).  xs: the layer's input
template <int T>
__global__ __launch_bounds__(64) void k_bcg_post(BCDims d, Segs sg, int rows, GradBufs gb, const float *__restrict__ xs) {
    using E = BCEnc<T>;
    constexpr int FE = E::FE, LDW = FE + 1;
    __shared__ float ldA[32 * LDW], ldB[32 * LDW];
    const int lane = threadIdx.x, h = lane >> 5, col = lane & 31;
    float *__restrict__ slice = gb.partials + (size_t)blockIdx.x * gb.G;
    const int total = rows * tiles_of(sg);
    for (int id = blockIdx.x; id < total; id += gridDim.x) {
        const TileAt ta = tile_at(sg, id);
        const Seg &s = sg.s[ta.second];
        const int qi = ta.tile * 32 + col;
        const bool live = qi < s.ntok;
        const size_t at = ((size_t)ta.b * d.L + s.tok0 + (live ? qi : s.ntok - 1)) * FE;
        const float *__restrict__ w = gb.blob + s.w, *__restrict__ wt = gb.WT + s.w;
        float *__restrict__ nw = slice + s.w + gb.nat_delta;
        f16v dout[T], zh[T], z[T], z1[T], g1[T], dt[T];
        float rstd;
        {
            f16v x[T], o[T];
            load_tok(gb.O + at, o, h);
            load_tok(xs + at, x, h);
            linear(o, w + E::S_OW, w + E::S_OB, z, lane, h);
#pragma unroll
            for (int t = 0; t < T; t++)
#pragma unroll
                for (int r = 0; r < 16; r++) z[t][r] = z[t][r] + x[t][r];
        }
        layer_norm_keep(z, zh, rstd, w + E::S_MG, w + E::S_MB, h);
        linear(z, w + E::S_W1, w + E::S_B1, z1, lane, h);
#pragma unroll
        for (int t = 0; t < T; t++)
#pragma unroll
            for (int r = 0; r < 16; r++) g1[t][r] = gelu_erf(z1[t][r]);
        load_tok(gb.dX + at, dout, h);
        if (!live) zero_tile(dout);
        linear_grads(nw + E::S_W2, nw + E::S_B2, dout, g1, ldA, ldB, lane, live);
        linear64_nb(dout, wt + E::S_W2, dt, lane);
#pragma unroll
        for (int t = 0; t < T; t++)
#pragma unroll
            for (int r = 0; r < 16; r++) dt[t][r] = dt[t][r] * gelu_erf_grad(z1[t][r]);
        linear_grads(nw + E::S_W1, nw + E::S_B1, dt, z, ldA, ldB, lane, live);
        linear64_nb(dt, wt + E::S_W1, g1, lane);  // g1: now the gradient at the MLP's LayerNorm output
        norm_grads(nw + E::S_MG, nw + E::S_MB, g1, zh, ldA, ldB, lane, live);
        layer_norm_back(g1, zh, rstd, w + E::S_MG, h);
#pragma unroll
        for (int t = 0; t < T; t++)
#pragma unroll
            for (int r = 0; r < 16; r++) dout[t][r] = dout[t][r] + g1[t][r];  // dy: the gradient at the attention residual's sum
        f16v o[T];
        load_tok(gb.O + at, o, h);  // (again: kept from the start it would cost 32 registers through the whole MLP)
        linear_grads(nw + E::S_OW, nw + E::S_OB, dout, o, ldA, ldB, lane, live);
        linear64_nb(dout, wt + E::S_OW, dt, lane);  // dO
        if (live) {
            store_tok(gb.dX + at, dout, h);
            store_tok(gb.dO + at, dt, h);
        }
    }
}

// grid (num_partials)
template <int T>
__global__ __launch_bounds__(64) void k_bcg_dq(BCDims d, Segs sg, int rows, GradBufs gb, const float *__restrict__ xs,
                                               const unsigned char *__restrict__ pm, const unsigned char *__restrict__ rm,
                                               const float *__restrict__ Kb, const float *__restrict__ Vb) {
    using E = BCEnc<T>;
    constexpr int FE = E::FE, HC = E::HC, LDW = FE + 1;
    __shared__ float ldA[32 * LDW], ldB[32 * LDW];
    __shared__ unsigned char msk[MAX_TOKENS];
    const int lane = threadIdx.x, h = lane >> 5, col = lane & 31;
    float *__restrict__ slice = gb.partials + (size_t)blockIdx.x * gb.G;
    const int total = rows * tiles_of(sg);
    for (int id = blockIdx.x; id < total; id += gridDim.x) {
        const TileAt ta = tile_at(sg, id);
        const Seg &s = sg.s[ta.second];
        const int ntok = s.ntok, b = ta.b;
        __syncthreads();
        for (int j = lane; j < ntok; j += 64) msk[j] = token_mask(d, pm, rm, b, s.tok0 + j);
        __syncthreads();
        const int qi = ta.tile * 32 + col;
        const bool live = qi < ntok;
        const size_t seg_at = ((size_t)b * d.L + s.tok0) * FE;
        const size_t tok = (size_t)b * d.L + s.tok0 + (live ? qi : ntok - 1), at = tok * FE;
        const float *__restrict__ w = gb.blob + s.w;
        float *__restrict__ nw = slice + s.w + gb.nat_delta;
        f16v hn[T], q[T], dao[T], dq[T];
        load_tok(xs + at, hn, h);
        layer_norm(hn, w + E::S_NG, w + E::S_NB, h);
        linear(hn, w + E::S_QW, w + E::S_QB, q, lane, h);
#pragma unroll
        for (int t = 0; t < T; t++)
#pragma unroll
            for (int r = 0; r < 16; r++) q[t][r] = q[t][r] * E::QSCALE;
        if (live) store_tok(gb.Q + at, q, h);
        load_tok(gb.dO + at, dao, h);
#pragma unroll
        for (int hd = 0; hd < 4; hd++) {
            const int t = T == 2 ? hd >> 1 : hd, rb = T == 2 ? 8 * (hd & 1) : 0;  // the head: registers rb .. rb + HC / 2 - 1 of tile t
            const float m = gb.ML[tok * 8 + hd], l = gb.ML[tok * 8 + 4 + hd];
            // D = sum_j P[j] dP[j] over the row's keys, as the softmax's backward sums it (with one unmasked key it IS that key's
            // dP, so dS is an exact 0 there): a first walk over the keys
            float D = 0.f;
            for (int kb = 0; kb < ntok; kb += 32) {
                const int key = min(kb + col, ntok - 1);
                const float *__restrict__ kp = Kb + seg_at + (size_t)key * FE + HC * hd + 4 * h;
                const float *__restrict__ vp = Vb + seg_at + (size_t)key * FE + HC * hd + 4 * h;
                f16v sc, dp;
#pragma unroll
                for (int r = 0; r < 16; r++) sc[r] = 0.f, dp[r] = 0.f;
                if constexpr (T == 2) {  // the 64-wide kernel's text as it was: as the loops below at HC = 16 it compiles to other code
                    const f4 k0 = *reinterpret_cast<const f4 *>(kp), k1 = *reinterpret_cast<const f4 *>(kp + 8);
                    const f4 v0 = *reinterpret_cast<const f4 *>(vp), v1 = *reinterpret_cast<const f4 *>(vp + 8);
#pragma unroll
                    for (int j = 0; j < 4; j++) sc = __builtin_amdgcn_mfma_f32_32x32x2f32(k0[j], q[t][rb + j], sc, 0, 0, 0);
#pragma unroll
                    for (int j = 0; j < 4; j++) sc = __builtin_amdgcn_mfma_f32_32x32x2f32(k1[j], q[t][rb + 4 + j], sc, 0, 0, 0);
#pragma unroll
                    for (int j = 0; j < 4; j++) dp = __builtin_amdgcn_mfma_f32_32x32x2f32(v0[j], dao[t][rb + j], dp, 0, 0, 0);
#pragma unroll
                    for (int j = 0; j < 4; j++) dp = __builtin_amdgcn_mfma_f32_32x32x2f32(v1[j], dao[t][rb + 4 + j], dp, 0, 0, 0);
                } else {
                    f4 f1[HC / 8], f2[HC / 8];
#pragma unroll
                    for (int g = 0; g < HC / 8; g++)
                        f1[g] = *reinterpret_cast<const f4 *>(kp + 8 * g), f2[g] = *reinterpret_cast<const f4 *>(vp + 8 * g);
#pragma unroll
                    for (int r = 0; r < HC / 2; r++) sc = __builtin_amdgcn_mfma_f32_32x32x2f32(f1[r >> 2][r & 3], q[t][rb + r], sc, 0, 0, 0);
#pragma unroll
                    for (int r = 0; r < HC / 2; r++) dp = __builtin_amdgcn_mfma_f32_32x32x2f32(f2[r >> 2][r & 3], dao[t][rb + r], dp, 0, 0, 0);
                }
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const int kk = kb + acc_row(r, h);
                    if (kk < ntok) D = D + (expf((msk[kk] ? -FLT_MAX : sc[r]) - m) / l) * dp[r];
                }
            }
            D = D + __shfl_xor(D, 32);
            if (live && h == 0) gb.D[tok * 4 + hd] = D;
            f16v acc;
#pragma unroll
            for (int r = 0; r < 16; r++) acc[r] = 0.f;
            for (int kb = 0; kb < ntok; kb += 32) {
                const int key = min(kb + col, ntok - 1);
                const float *__restrict__ kp = Kb + seg_at + (size_t)key * FE + HC * hd + 4 * h;
                const float *__restrict__ vp = Vb + seg_at + (size_t)key * FE + HC * hd + 4 * h;
                f16v sc, dp;
#pragma unroll
                for (int r = 0; r < 16; r++) sc[r] = 0.f, dp[r] = 0.f;
                if constexpr (T == 2) {  // the 64-wide kernel's text as it was: as the loops below at HC = 16 it compiles to other code
                    const f4 k0 = *reinterpret_cast<const f4 *>(kp), k1 = *reinterpret_cast<const f4 *>(kp + 8);
                    const f4 v0 = *reinterpret_cast<const f4 *>(vp), v1 = *reinterpret_cast<const f4 *>(vp + 8);
#pragma unroll
                    for (int j = 0; j < 4; j++) sc = __builtin_amdgcn_mfma_f32_32x32x2f32(k0[j], q[t][rb + j], sc, 0, 0, 0);
#pragma unroll
                    for (int j = 0; j < 4; j++) sc = __builtin_amdgcn_mfma_f32_32x32x2f32(k1[j], q[t][rb + 4 + j], sc, 0, 0, 0);
#pragma unroll
                    for (int j = 0; j < 4; j++) dp = __builtin_amdgcn_mfma_f32_32x32x2f32(v0[j], dao[t][rb + j], dp, 0, 0, 0);
#pragma unroll
                    for (int j = 0; j < 4; j++) dp = __builtin_amdgcn_mfma_f32_32x32x2f32(v1[j], dao[t][rb + 4 + j], dp, 0, 0, 0);
                } else {
                    f4 f1[HC / 8], f2[HC / 8];
#pragma unroll
                    for (int g = 0; g < HC / 8; g++)
                        f1[g] = *reinterpret_cast<const f4 *>(kp + 8 * g), f2[g] = *reinterpret_cast<const f4 *>(vp + 8 * g);
#pragma unroll
                    for (int r = 0; r < HC / 2; r++) sc = __builtin_amdgcn_mfma_f32_32x32x2f32(f1[r >> 2][r & 3], q[t][rb + r], sc, 0, 0, 0);
#pragma unroll
                    for (int r = 0; r < HC / 2; r++) dp = __builtin_amdgcn_mfma_f32_32x32x2f32(f2[r >> 2][r & 3], dao[t][rb + r], dp, 0, 0, 0);
                }
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const int kk = kb + acc_row(r, h);
                    float ds = 0.f;
                    if (kk < ntok && !msk[kk]) ds = (expf(sc[r] - m) / l) * (dp[r] - D);  // a masked score receives nothing
                    sc[r] = ds;
                }
                // dQ^T[channel][query] += K^T dS^T: at 64 rows 16 .. 31 repeat the channels, as the forward's O^T; at 128 all 32 rows are the head's
                const float *__restrict__ kc = Kb + seg_at + HC * hd + (col & (HC - 1));
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const int vk = min(kb + acc_row(r, h), ntok - 1);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(kc[(size_t)vk * FE], sc[r], acc, 0, 0, 0);
                }
            }
#pragma unroll
            for (int r = 0; r < HC / 2; r++) dq[t][rb + r] = live ? acc[r] * E::QSCALE : 0.f;
        }
        if (live) store_tok(gb.dQ + at, dq, h);
        linear_grads(nw + E::S_QW, nw + E::S_QB, dq, hn, ldA, ldB, lane, live);
    }
}

// grid (num_partials)
template <int T>
__global__ __launch_bounds__(64) void k_bcg_dkv(BCDims d, Segs sg, int rows, GradBufs gb, const float *__restrict__ xs,
                                                const unsigned char *__restrict__ pm, const unsigned char *__restrict__ rm,
                                                const float *__restrict__ Kb, const float *__restrict__ Vb) {
    using E = BCEnc<T>;
    constexpr int FE = E::FE, HC = E::HC, LDW = FE + 1;
    __shared__ float ldA[32 * LDW], ldB[32 * LDW];
    const int lane = threadIdx.x, h = lane >> 5, col = lane & 31;
    float *__restrict__ slice = gb.partials + (size_t)blockIdx.x * gb.G;
    const int total = rows * tiles_of(sg);
    for (int id = blockIdx.x; id < total; id += gridDim.x) {
        const TileAt ta = tile_at(sg, id);
        const Seg &s = sg.s[ta.second];
        const int ntok = s.ntok, b = ta.b;
        const int ki = ta.tile * 32 + col;
        const bool live = ki < ntok;
        const int kc = live ? ki : ntok - 1;
        const size_t seg_tok = (size_t)b * d.L + s.tok0, seg_at = seg_tok * FE, at = seg_at + (size_t)kc * FE;
        const bool kmask = token_mask(d, pm, rm, b, s.tok0 + kc) != 0;
        const float *__restrict__ w = gb.blob + s.w, *__restrict__ wt = gb.WT + s.w;
        float *__restrict__ nw = slice + s.w + gb.nat_delta;
        f16v kt[T], vt[T], dk[T], dv[T];
        load_tok(Kb + at, kt, h);
        load_tok(Vb + at, vt, h);
#pragma unroll
        for (int hd = 0; hd < 4; hd++) {
            const int t = T == 2 ? hd >> 1 : hd, rb = T == 2 ? 8 * (hd & 1) : 0;  // the head: registers rb .. rb + HC / 2 - 1 of tile t
            f16v ak, av;
#pragma unroll
            for (int r = 0; r < 16; r++) ak[r] = 0.f, av[r] = 0.f;
            for (int qb = 0; qb < ntok; qb += 32) {
                const int qrow = min(qb + col, ntok - 1);
                const float *__restrict__ qp = gb.Q + seg_at + (size_t)qrow * FE + HC * hd + 4 * h;
                const float *__restrict__ ap = gb.dO + seg_at + (size_t)qrow * FE + HC * hd + 4 * h;
                // S[query][key] and dP[query][key]: the query in the registers, the key on the lane
                f16v sc, dp;
#pragma unroll
                for (int r = 0; r < 16; r++) sc[r] = 0.f, dp[r] = 0.f;
                if constexpr (T == 2) {  // the 64-wide kernel's text as it was: as the loops below at HC = 16 it compiles to other code
                    const f4 q0 = *reinterpret_cast<const f4 *>(qp), q1 = *reinterpret_cast<const f4 *>(qp + 8);
                    const f4 a0 = *reinterpret_cast<const f4 *>(ap), a1 = *reinterpret_cast<const f4 *>(ap + 8);
#pragma unroll
                    for (int j = 0; j < 4; j++) sc = __builtin_amdgcn_mfma_f32_32x32x2f32(q0[j], kt[t][rb + j], sc, 0, 0, 0);
#pragma unroll
                    for (int j = 0; j < 4; j++) sc = __builtin_amdgcn_mfma_f32_32x32x2f32(q1[j], kt[t][rb + 4 + j], sc, 0, 0, 0);
#pragma unroll
                    for (int j = 0; j < 4; j++) dp = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[j], vt[t][rb + j], dp, 0, 0, 0);
#pragma unroll
                    for (int j = 0; j < 4; j++) dp = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[j], vt[t][rb + 4 + j], dp, 0, 0, 0);
                } else {
                    f4 f1[HC / 8], f2[HC / 8];
#pragma unroll
                    for (int g = 0; g < HC / 8; g++)
                        f1[g] = *reinterpret_cast<const f4 *>(qp + 8 * g), f2[g] = *reinterpret_cast<const f4 *>(ap + 8 * g);
#pragma unroll
                    for (int r = 0; r < HC / 2; r++) sc = __builtin_amdgcn_mfma_f32_32x32x2f32(f1[r >> 2][r & 3], kt[t][rb + r], sc, 0, 0, 0);
#pragma unroll
                    for (int r = 0; r < HC / 2; r++) dp = __builtin_amdgcn_mfma_f32_32x32x2f32(f2[r >> 2][r & 3], vt[t][rb + r], dp, 0, 0, 0);
                }
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const int qq = qb + acc_row(r, h);
                    float p = 0.f, ds = 0.f;
                    if (qq < ntok) {
                        const size_t qt = seg_tok + qq;
                        const float m = gb.ML[qt * 8 + hd], l = gb.ML[qt * 8 + 4 + hd];
                        p = expf((kmask ? -FLT_MAX : sc[r]) - m) / l;
                        if (!kmask) ds = p * (dp[r] - gb.D[qt * 4 + hd]);
                    }
                    sc[r] = p, dp[r] = ds;
                }
                // dV^T[channel][key] += dO^T P and dK^T[channel][key] += Q^T dS: the A operand walks the queries
                const float *__restrict__ ac = gb.dO + seg_at + HC * hd + (col & (HC - 1));
                const float *__restrict__ qc = gb.Q + seg_at + HC * hd + (col & (HC - 1));
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const int qk = min(qb + acc_row(r, h), ntok - 1);
                    av = __builtin_amdgcn_mfma_f32_32x32x2f32(ac[(size_t)qk * FE], sc[r], av, 0, 0, 0);
                    ak = __builtin_amdgcn_mfma_f32_32x32x2f32(qc[(size_t)qk * FE], dp[r], ak, 0, 0, 0);
                }
            }
#pragma unroll
            for (int r = 0; r < HC / 2; r++) dk[t][rb + r] = live ? ak[r] : 0.f, dv[t][rb + r] = live ? av[r] : 0.f;
        }
        f16v hn[T], xh[T], dh[T], tmp[T];
        float rstd;
        load_tok(xs + at, hn, h);
        layer_norm_keep(hn, xh, rstd, w + E::S_NG, w + E::S_NB, h);
        linear_grads(nw + E::S_KW, nw + E::S_KB, dk, hn, ldA, ldB, lane, live);
        linear_grads(nw + E::S_VW, nw + E::S_VB, dv, hn, ldA, ldB, lane, live);
        linear64_nb(dk, wt + E::S_KW, dh, lane);
        linear64_nb(dv, wt + E::S_VW, tmp, lane);
#pragma unroll
        for (int t = 0; t < T; t++)
#pragma unroll
            for (int r = 0; r < 16; r++) dh[t][r] = dh[t][r] + tmp[t][r];
        load_tok(gb.dQ + at, dk, h);  // dk: now this token's dQ
        if (!live) zero_tile(dk);
        linear64_nb(dk, wt + E::S_QW, tmp, lane);
#pragma unroll
        for (int t = 0; t < T; t++)
#pragma unroll
            for (int r = 0; r < 16; r++) dh[t][r] = dh[t][r] + tmp[t][r];
        norm_grads(nw + E::S_NG, nw + E::S_NB, dh, xh, ldA, ldB, lane, live);
        layer_norm_back(dh, xh, rstd, w + E::S_NG, h);
        load_tok(gb.dX + at, tmp, h);  // the residual's share, k_bcg_post's
#pragma unroll
        for (int t = 0; t < T; t++)
#pragma unroll
            for (int r = 0; r < 16; r++) dh[t][r] = dh[t][r] + tmp[t][r];
        if (live) store_tok(gb.dX + at, dh, h);
    }
}

// the keys and values of the two cross attentions: dK in gb.dO, dV in gb.dQ (k_bcg_head wrote them).  grid (num_partials)
template <int T>
__global__ __launch_bounds__(64) void k_bcg_kvx(BCDims d, Segs sg, int rows, GradBufs gb, const float *__restrict__ X) {
    using E = BCEnc<T>;
    constexpr int FE = E::FE, LDW = FE + 1;
    __shared__ float ldA[32 * LDW], ldB[32 * LDW];
    const int lane = threadIdx.x, h = lane >> 5, col = lane & 31;
    float *__restrict__ slice = gb.partials + (size_t)blockIdx.x * gb.G;
    const int total = rows * tiles_of(sg);
    for (int id = blockIdx.x; id < total; id += gridDim.x) {
        const TileAt ta = tile_at(sg, id);
        const Seg &s = sg.s[ta.second];
        const int ki = ta.tile * 32 + col;
        const bool live = ki < s.ntok;
        const size_t at = ((size_t)ta.b * d.L + s.tok0 + (live ? ki : s.ntok - 1)) * FE;
        // the Seg of a cross attention holds its fields one by one
        float *__restrict__ ng = slice + gb.nat_delta;
        f16v hn[T], xh[T], dk[T], dv[T], dh[T], tmp[T];
        float rstd;
        load_tok(X + at, hn, h);
        layer_norm_keep(hn, xh, rstd, gb.blob + s.ng, gb.blob + s.nb, h);
        load_tok(gb.dO + at, dk, h);
        load_tok(gb.dQ + at, dv, h);
        if (!live) zero_tile(dk), zero_tile(dv);
        linear_grads(ng + s.kw, ng + s.kb, dk, hn, ldA, ldB, lane, live);
        linear_grads(ng + s.vw, ng + s.vb, dv, hn, ldA, ldB, lane, live);
        linear64_nb(dk, gb.WT + s.kw, dh, lane);
        linear64_nb(dv, gb.WT + s.vw, tmp, lane);
#pragma unroll
        for (int t = 0; t < T; t++)
#pragma unroll
            for (int r = 0; r < 16; r++) dh[t][r] = dh[t][r] + tmp[t][r];
        norm_grads(ng + s.ng, ng + s.nb, dh, xh, ldA, ldB, lane, live);
        layer_norm_back(dh, xh, rstd, gb.blob + s.ng, h);
        if (live) store_tok(gb.dX + at, dh, h);
    }
}

// ---- the embedders

struct EmbedAt {
    int kind, e, count;
};

__device__ __forceinline__ EmbedAt embed_at(const BCDims &d, int tile) {
    const int ptiles = (d.A - 1 + 31) / 32;
    EmbedAt a;
    a.kind = tile == 0 ? 0 : tile <= ptiles ? 1 : 2;
    a.count = a.kind == 0 ? 1 : a.kind == 1 ? d.A - 1 : ROADS;
    a.e = a.kind == 0 ? 0 : a.kind == 1 ? (tile - 1) * 32 : (tile - 1 - ptiles) * 32;
    return a;
}

// the embedder's activation after `upto` of its four (Linear, LayerNorm, tanh) layers, as k_bc_embed computes it
template <int T>
__device__ __forceinline__ void embed_forward(const BCDims &d, int kind, int ec, const float *__restrict__ x, const float *__restrict__ w0,
                                              const float *__restrict__ rest, int upto, f16v (&a)[T], int lane, int h) {
    constexpr int FE = BCEnc<T>::FE, W = BCEnc<T>::W;
    f16v o[T];
    if (kind == 2)
        embed_first<ROAD_K>(x, d.D, d.R, EGO_K + PARTNER_K * (d.A - 1), ec, w0, rest, a, lane, h);
    else
        embed_first<PARTNER_K>(x, d.D, d.R, kind == 0 ? 0 : EGO_K, ec, w0, rest, a, lane, h);
    layer_norm(a, rest + FE, rest + 2 * FE, h);
#pragma unroll
    for (int t = 0; t < T; t++)
#pragma unroll
        for (int r = 0; r < 16; r++) a[t][r] = tanhf(a[t][r]);
    for (int i = 0; i + 1 < upto; i++) {
        const float *__restrict__ w = rest + 3 * FE + i * (W + 3 * FE);
        linear(a, w, w + W, o, lane, h);
        layer_norm(o, w + W + FE, w + W + 2 * FE, h);
#pragma unroll
        for (int t = 0; t < T; t++)
#pragma unroll
            for (int r = 0; r < 16; r++) a[t][r] = tanhf(o[t][r]);
    }
}

// grid (num_partials).  L: the blob's layout, N: the gradient's
template <int T>
__global__ __launch_bounds__(64) void k_bcg_embed(BCDims d, BCLayout L, BCLayout N, int rows, GradBufs gb, const float *__restrict__ obs) {
    using E = BCEnc<T>;
    constexpr int FE = E::FE, W = E::W, LDW = FE + 1;
    __shared__ float ldA[32 * LDW], ldB[32 * LDW], ldX[32 * LXW];
    const int lane = threadIdx.x, h = lane >> 5, col = lane & 31;
    float *__restrict__ slice = gb.partials + (size_t)blockIdx.x * gb.G;
    const int etiles = 1 + (d.A - 1 + 31) / 32 + (ROADS + 31) / 32;
    const int total = rows * etiles;
    for (int id = blockIdx.x; id < total; id += gridDim.x) {
        const int b = id / etiles;
        const EmbedAt ea = embed_at(d, id % etiles);
        const int kind = ea.kind, e = ea.e + col;
        const bool live = e < ea.count;
        const int ec = live ? e : ea.count - 1;
        const float *__restrict__ x = obs + (size_t)b * d.R * d.D;
        const float *__restrict__ w0 = gb.blob + L.net_w0[kind], *__restrict__ rest = gb.blob + L.net_rest[kind];
        float *__restrict__ nrest = slice + N.net_rest[kind];
        const int tok = (kind == 0 ? 0 : kind == 1 ? 1 : d.A) + ec;
        f16v dcur[T], a[T], z[T], xh[T];
        float rstd;
        load_tok(gb.dX + ((size_t)b * d.L + tok) * FE, dcur, h);
        if (!live) zero_tile(dcur);
        for (int i = 3; i >= 1; i--) {
            embed_forward(d, kind, ec, x, w0, rest, i, a, lane, h);  // the input of layer i
            const float *__restrict__ w = rest + 3 * FE + (i - 1) * (W + 3 * FE);
            float *__restrict__ nwl = nrest + 3 * FE + (i - 1) * (W + 3 * FE);
            linear(a, w, w + W, z, lane, h);
            layer_norm_keep(z, xh, rstd, w + W + FE, w + W + 2 * FE, h);
#pragma unroll
            for (int t = 0; t < T; t++)
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const float th = tanhf(z[t][r]);
                    dcur[t][r] = dcur[t][r] * (1.f - th * th);
                }
            norm_grads(nwl + W + FE, nwl + W + 2 * FE, dcur, xh, ldA, ldB, lane, live);
            layer_norm_back(dcur, xh, rstd, w + W + FE, h);
            linear_grads(nwl, nwl + W, dcur, a, ldA, ldB, lane, live);
            linear64_nb(dcur, gb.WT + L.net_rest[kind] + 3 * FE + (i - 1) * (W + 3 * FE), z, lane);
#pragma unroll
            for (int t = 0; t < T; t++) dcur[t] = z[t];
        }
        // the first layer: its input is the token's R rows of obs
        const int KT = kind == 2 ? ROAD_K : PARTNER_K, kin = KT * d.R;
        const int base = kind == 0 ? 0 : kind == 1 ? EGO_K : EGO_K + PARTNER_K * (d.A - 1);
        if (kind == 2)
            embed_first<ROAD_K>(x, d.D, d.R, base, ec, w0, rest, z, lane, h);
        else
            embed_first<PARTNER_K>(x, d.D, d.R, base, ec, w0, rest, z, lane, h);
        layer_norm_keep(z, xh, rstd, rest + FE, rest + 2 * FE, h);
#pragma unroll
        for (int t = 0; t < T; t++)
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const float th = tanhf(z[t][r]);
                dcur[t][r] = dcur[t][r] * (1.f - th * th);
            }
        norm_grads(nrest + FE, nrest + 2 * FE, dcur, xh, ldA, ldB, lane, live);
        layer_norm_back(dcur, xh, rstd, rest + FE, h);
        __syncthreads();
        tile_to_lds(ldA, dcur, col, h, live);
        const int kpad = (kin + 31) & ~31;
        for (int k = h; k < kpad; k += 2)
            ldX[col * LXW + k] = (live && k < kin) ? x[(size_t)(k / KT) * d.D + base + ec * KT + (k % KT)] : 0.f;
        __syncthreads();
        accum_dw<T>(slice + N.net_w0[kind], kin, ldA, ldX, LXW, lane);
        accum_vec<T>(nrest, ldA, lane);
    }
}

// ---- the head: a wave per row, lane per feature

__device__ __forceinline__ float wave_ln_keep(float a, float &xh, float &rstd, const float *__restrict__ g, const float *__restrict__ be,
                                              int lane) {
    const float mean = wave_sum(a) * (1.f / 64.f);
    const float dlt = a - mean;
    rstd = 1.f / sqrtf(wave_sum(dlt * dlt) * (1.f / 64.f) + LN_EPS);
    xh = dlt * rstd;
    return xh * g[lane] + be[lane];
}

__device__ __forceinline__ float wave_ln_back(float dz, float xh, float rstd, float g) {
    const float dd = dz * g;
    const float m1 = wave_sum(dd) * (1.f / 64.f), m2 = wave_sum(dd * xh) * (1.f / 64.f);
    return rstd * ((dd - m1) - xh * m2);
}

// out[lane] = sum_o wt[o][lane] v[o], ascending o; wt is the weight in its natural layout [out 64][in 64]
__device__ __forceinline__ float matvec64_t(const float *__restrict__ wt, float v, int lane) {
    float o = 0.f;
    for (int k = 0; k < F; k++) o = o + wt[k * F + lane] * __shfl(v, k);
    return o;
}

// w[o][lane] += dy[o] x[lane] for a [64][64] weight of this workgroup's slice; b[lane] += dy[lane]
__device__ __forceinline__ void outer64(float *__restrict__ w, float *__restrict__ b, float dy, float x, int lane) {
    for (int o = 0; o < F; o++) w[o * F + lane] = w[o * F + lane] + __shfl(dy, o) * x;
    b[lane] = b[lane] + dy;
}

struct CrossKeep {
    float xhq, rstdq, qn, o, y, zh, rstdm, zn, z1, g1;
};

struct HeadGradArgs {
    int head_layers, C;
    float clip;
    const float *expert, *gnll;
};

// network_dim 64.  grid (num_partials).  Writes dX[b][token 0], dK (gb.dO) and dV (gb.dQ) of every cross-attention key
__global__ __launch_bounds__(64) void k_bcg_head(BCDims d, BCLayout L, HeadGradArgs a, int rows, GradBufs gb,
                                                 const unsigned char *__restrict__ pm, const unsigned char *__restrict__ rm,
                                                 const float *__restrict__ X, const float *__restrict__ Kb,
                                                 const float *__restrict__ Vb) {
    using E = BCEnc<2>;
    __shared__ float prob[2][4][ROADS];
    __shared__ float ds[4][ROADS];
    __shared__ float qs[2][F];
    __shared__ float ctx[E::CTX], dctx[E::CTX];
    __shared__ float vec[F];
    __shared__ float raw[MAX_HEAD_OUT], draw[MAX_HEAD_OUT];
    __shared__ float hin[5][F], pre[5][F];
    const int lane = threadIdx.x, hd = lane >> 4;
    const float *__restrict__ blob = gb.blob;
    float *__restrict__ slice = gb.partials + (size_t)blockIdx.x * gb.G + gb.nat_delta;  // indexed by blob offsets
    for (int b = blockIdx.x; b < rows; b += gridDim.x) {
        __syncthreads();
        const size_t base = (size_t)b * d.L * F;
        const float xq = X[base + lane];
        ctx[lane] = xq;
        CrossKeep keep[2];
#pragma unroll
        for (int ci = 0; ci < 2; ci++) {
            CrossKeep &k = keep[ci];
            const int tok0 = ci ? d.A : 1, nk = ci ? ROADS : d.A - 1;
            const float *__restrict__ w = blob + L.cross[ci];
            const float *__restrict__ wb = w + E::C_BODY;
            k.qn = wave_ln_keep(xq, k.xhq, k.rstdq, w + E::C_QG, w + E::C_QB, lane);
            qs[ci][lane] = matvec64(wb + E::S_QW, wb + E::S_QB, k.qn, lane) * 0.25f;
            __syncthreads();
            for (int j = lane; j < nk; j += 64) {
                const float *__restrict__ kp = Kb + base + (size_t)(tok0 + j) * F;
                const bool masked = token_mask(d, pm, rm, b, tok0 + j) != 0;
                for (int g = 0; g < 4; g++) {
                    float s = 0.f;
                    for (int c = 0; c < 16; c++) s = s + qs[ci][16 * g + c] * kp[16 * g + c];
                    prob[ci][g][j] = masked ? -FLT_MAX : s;
                }
            }
            __syncthreads();
            for (int g = 0; g < 4; g++) {
                float m = -INFINITY;
                for (int j = lane; j < nk; j += 64) m = fmaxf(m, prob[ci][g][j]);
                m = wave_max(m);
                float ps = 0.f;
                for (int j = lane; j < nk; j += 64) {
                    const float p = expf(prob[ci][g][j] - m);
                    prob[ci][g][j] = p;
                    ps = ps + p;
                }
                const float S = wave_sum(ps);
                for (int j = lane; j < nk; j += 64) prob[ci][g][j] = prob[ci][g][j] / S;
            }
            __syncthreads();
            float o = 0.f;
            for (int j = 0; j < nk; j++) o = o + prob[ci][hd][j] * Vb[base + (size_t)(tok0 + j) * F + lane];
            k.o = o;
            k.y = matvec64(wb + E::S_OW, wb + E::S_OB, o, lane) + xq;
            k.zn = wave_ln_keep(k.y, k.zh, k.rstdm, wb + E::S_MG, wb + E::S_MB, lane);
            k.z1 = matvec64(wb + E::S_W1, wb + E::S_B1, k.zn, lane);
            k.g1 = gelu_erf(k.z1);
            ctx[F * (1 + ci) + lane] = k.y + matvec64(wb + E::S_W2, wb + E::S_B2, k.g1, lane);
            __syncthreads();
        }
        // the GMM head, forward
        float hcur = blob[L.head_in_b + lane];
        for (int k = 0; k < E::CTX; k++) hcur = hcur + blob[L.head_in_w + k * F + lane] * ctx[k];
        pre[0][lane] = hcur;
        hcur = fmaxf(hcur, 0.f);
        for (int i = 0; i < a.head_layers; i++) {
            const float *__restrict__ w = blob + L.head_res + i * (W64 + F);
            hin[i][lane] = hcur;
            const float pr = matvec64(w, w + W64, hcur, lane);
            pre[1 + i][lane] = pr;
            hcur = hcur + fmaxf(pr, 0.f);
        }
        hin[a.head_layers][lane] = hcur;
        vec[lane] = hcur;
        __syncthreads();
        const int C = a.C, NO = 7 * C;
        for (int o = lane; o < NO; o += 64) {
            float r = blob[L.head_b + o];
            for (int k = 0; k < F; k++) r = r + blob[L.head_w + k * NO + o] * vec[k];
            raw[o] = r;
        }
        __syncthreads();
        // the rule's gradient, scaled by the row's upstream gradient
        {
            auto load = [&](int k) { return raw[k]; };
            const float e[3] = {a.expert[(size_t)b * 3], a.expert[(size_t)b * 3 + 1], a.expert[(size_t)b * 3 + 2]};
            const bc_rule::Weights ws = bc_rule::weight_stats(C, load);
            const bc_grad_rule::Stats st = bc_grad_rule::stats(C, load, a.clip, ws, e);
            const float gn = a.gnll[b];
            for (int o = lane; o < NO; o += 64) draw[o] = bc_grad_rule::grad(C, load, a.clip, ws, e, st, o) * gn;
        }
        __syncthreads();
        // head.head
        float dh = 0.f;
        for (int o = 0; o < NO; o++) {
            slice[L.head_w + o * F + lane] = slice[L.head_w + o * F + lane] + draw[o] * hcur;
            dh = dh + gb.WT[L.head_w + o * F + lane] * draw[o];
        }
        for (int o = lane; o < NO; o += 64) slice[L.head_b + o] = slice[L.head_b + o] + draw[o];
        for (int i = a.head_layers - 1; i >= 0; i--) {
            const int off = L.head_res + i * (W64 + F);
            const float dp = pre[1 + i][lane] > 0.f ? dh : 0.f;
            outer64(slice + off, slice + off + W64, dp, hin[i][lane], lane);
            dh = dh + matvec64_t(gb.WT + off, dp, lane);
        }
        {
            const float dp = pre[0][lane] > 0.f ? dh : 0.f;
            float dc[3] = {0.f, 0.f, 0.f};
            for (int o = 0; o < F; o++) {
                const float dpo = __shfl(dp, o);
#pragma unroll
                for (int j = 0; j < 3; j++) {
                    const int at = L.head_in_w + o * E::CTX + F * j + lane;
                    slice[at] = slice[at] + dpo * ctx[F * j + lane];
                    dc[j] = dc[j] + gb.WT[at] * dpo;
                }
            }
            slice[L.head_in_b + lane] = slice[L.head_in_b + lane] + dp;
#pragma unroll
            for (int j = 0; j < 3; j++) dctx[F * j + lane] = dc[j];
        }
        __syncthreads();
        float dxq = dctx[lane];
#pragma unroll
        for (int ci = 0; ci < 2; ci++) {
            const CrossKeep &k = keep[ci];
            const int tok0 = ci ? d.A : 1, nk = ci ? ROADS : d.A - 1;
            const int cw = L.cross[ci], cb = cw + E::C_BODY;
            const float *__restrict__ wtb = gb.WT + cb;
            float *__restrict__ nb = slice + cb, *__restrict__ nw = slice + cw;
            const float dout = dctx[F * (1 + ci) + lane];
            outer64(nb + E::S_W2, nb + E::S_B2, dout, k.g1, lane);
            const float dz1 = matvec64_t(wtb + E::S_W2, dout, lane) * gelu_erf_grad(k.z1);
            outer64(nb + E::S_W1, nb + E::S_B1, dz1, k.zn, lane);
            const float dzn = matvec64_t(wtb + E::S_W1, dz1, lane);
            nb[E::S_MG + lane] = nb[E::S_MG + lane] + dzn * k.zh;
            nb[E::S_MB + lane] = nb[E::S_MB + lane] + dzn;
            const float dy = dout + wave_ln_back(dzn, k.zh, k.rstdm, blob[cb + E::S_MG + lane]);
            outer64(nb + E::S_OW, nb + E::S_OB, dy, k.o, lane);
            const float dao = matvec64_t(wtb + E::S_OW, dy, lane);
            dxq = dxq + dy;
            // the one-query attention
            __syncthreads();
            vec[lane] = dao;
            __syncthreads();
            for (int j = lane; j < nk; j += 64) {
                const float *__restrict__ vp = Vb + base + (size_t)(tok0 + j) * F;
                for (int g = 0; g < 4; g++) {
                    float s = 0.f;
                    for (int c = 0; c < 16; c++) s = s + vec[16 * g + c] * vp[16 * g + c];
                    ds[g][j] = s;  // dP
                }
            }
            __syncthreads();
            for (int g = 0; g < 4; g++) {
                float part = 0.f;
                for (int j = lane; j < nk; j += 64) part = part + prob[ci][g][j] * ds[g][j];
                const float D = wave_sum(part);
                for (int j = lane; j < nk; j += 64) {
                    const bool masked = token_mask(d, pm, rm, b, tok0 + j) != 0;
                    ds[g][j] = masked ? 0.f : prob[ci][g][j] * (ds[g][j] - D);  // a masked score receives nothing
                }
            }
            __syncthreads();
            float dq = 0.f;
            const float qv = qs[ci][lane];
            for (int j = 0; j < nk; j++) {
                const size_t at = base + (size_t)(tok0 + j) * F + lane;
                const float dsj = ds[hd][j];
                gb.dQ[at] = prob[ci][hd][j] * dao;  // dV
                gb.dO[at] = dsj * qv;               // dK
                dq = dq + dsj * Kb[at];
            }
            dq = dq * 0.25f;
            outer64(nb + E::S_QW, nb + E::S_QB, dq, k.qn, lane);
            const float dqn = matvec64_t(wtb + E::S_QW, dq, lane);
            nw[E::C_QG + lane] = nw[E::C_QG + lane] + dqn * k.xhq;
            nw[E::C_QB + lane] = nw[E::C_QB + lane] + dqn;
            dxq = dxq + wave_ln_back(dqn, k.xhq, k.rstdq, blob[cw + E::C_QG + lane]);
        }
        gb.dX[base + lane] = dxq;
    }
}

// ---- the head at network_dim 128: a workgroup of 128 threads per row, a thread per encoder feature, as k_bc_head_block.
// Every sum across the two waves goes through LDS and is summed by its owner in ascending order (block_ln128's way: every
// thread sums the 128 entries itself).  The 64-wide GMM head, bc_rule.hpp and bc_grad_rule.hpp run on threads 0 .. 63, which
// are wave 0, on k_bcg_head's own shuffles.  Written out beside k_bcg_head, as the forward's two head kernels are.

// block_ln128 of bc_tile.hpp (the same operations in the same order), keeping the normalised value and 1 / std
__device__ __forceinline__ float block_ln128_keep(float a, float &xh, float &rstd, const float *__restrict__ g,
                                                  const float *__restrict__ be, int tid, float *buf) {
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
    rstd = 1.f / sqrtf(sq * (1.f / 128.f) + LN_EPS);
    xh = dlt * rstd;
    return xh * g[tid] + be[tid];
}

__device__ __forceinline__ float block_sum128(float v, int tid, float *buf) {
    buf[tid] = v;
    __syncthreads();
    float s = 0.f;
    for (int k = 0; k < 128; k++) s = s + buf[k];
    __syncthreads();
    return s;
}

__device__ __forceinline__ float block_ln128_back(float dz, float xh, float rstd, float g, int tid, float *buf) {
    const float dd = dz * g;
    const float m1 = block_sum128(dd, tid, buf) * (1.f / 128.f), m2 = block_sum128(dd * xh, tid, buf) * (1.f / 128.f);
    return rstd * ((dd - m1) - xh * m2);
}

// a [128][128] Linear of the one token, backward: w[o][tid] += dy[o] x[tid] and b[tid] += dy[tid] in this workgroup's slice;
// returns sum_o wt[o][tid] dy[o], ascending o (wt: the weight in its natural layout [out][in])
__device__ __forceinline__ float block_linear128_back(float *__restrict__ w, float *__restrict__ b, const float *__restrict__ wt,
                                                      float dy, float x, int tid, float *buf) {
    buf[tid] = dy;
    __syncthreads();
    float o = 0.f;
    for (int k = 0; k < 128; k++) {
        const float dk = buf[k];
        w[k * 128 + tid] = w[k * 128 + tid] + dk * x;
        o = o + wt[k * 128 + tid] * dk;
    }
    b[tid] = b[tid] + dy;
    __syncthreads();
    return o;
}

// grid (num_partials), 128 threads.  Writes dX[b][token 0], dK (gb.dO) and dV (gb.dQ) of every cross-attention key
__global__ __launch_bounds__(128) void k_bcg_head_block(BCDims d, BCLayout L, HeadGradArgs a, int rows, GradBufs gb,
                                                        const unsigned char *__restrict__ pm, const unsigned char *__restrict__ rm,
                                                        const float *__restrict__ X, const float *__restrict__ Kb,
                                                        const float *__restrict__ Vb) {
    using E = BCEnc<4>;
    constexpr int FE = E::FE;
    __shared__ float prob[2][4][ROADS];
    __shared__ float ds[4][ROADS];
    __shared__ float qs[2][FE];
    __shared__ float ctx[E::CTX], dctx[E::CTX];
    __shared__ float vec[FE];
    __shared__ float raw[MAX_HEAD_OUT], draw[MAX_HEAD_OUT];
    __shared__ float hin[5][F], pre[5][F];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, hd = tid >> 5;
    const float *__restrict__ blob = gb.blob;
    float *__restrict__ slice = gb.partials + (size_t)blockIdx.x * gb.G + gb.nat_delta;  // indexed by blob offsets
    for (int b = blockIdx.x; b < rows; b += gridDim.x) {
        __syncthreads();
        const size_t base = (size_t)b * d.L * FE;
        const float xq = X[base + tid];
        ctx[tid] = xq;
        CrossKeep keep[2];
#pragma unroll
        for (int ci = 0; ci < 2; ci++) {
            CrossKeep &k = keep[ci];
            const int tok0 = ci ? d.A : 1, nk = ci ? ROADS : d.A - 1;
            const float *__restrict__ w = blob + L.cross[ci];
            const float *__restrict__ wb = w + E::C_BODY;
            k.qn = block_ln128_keep(xq, k.xhq, k.rstdq, w + E::C_QG, w + E::C_QB, tid, vec);
            qs[ci][tid] = block_matvec128(wb + E::S_QW, wb + E::S_QB, k.qn, tid, vec) * E::QSCALE;
            __syncthreads();
            for (int j = tid; j < nk; j += 128) {
                const float *__restrict__ kp = Kb + base + (size_t)(tok0 + j) * FE;
                const bool masked = token_mask(d, pm, rm, b, tok0 + j) != 0;
                for (int g = 0; g < 4; g++) {
                    float s = 0.f;
                    for (int c = 0; c < 32; c++) s = s + qs[ci][32 * g + c] * kp[32 * g + c];
                    prob[ci][g][j] = masked ? -FLT_MAX : s;
                }
            }
            __syncthreads();
            for (int g = 2 * wv; g < 2 * wv + 2; g++) {  // a wave per two heads, its lanes stride the keys
                float m = -INFINITY;
                for (int j = lane; j < nk; j += 64) m = fmaxf(m, prob[ci][g][j]);
                m = wave_max(m);
                float ps = 0.f;
                for (int j = lane; j < nk; j += 64) {
                    const float p = expf(prob[ci][g][j] - m);
                    prob[ci][g][j] = p;
                    ps = ps + p;
                }
                const float S = wave_sum(ps);
                for (int j = lane; j < nk; j += 64) prob[ci][g][j] = prob[ci][g][j] / S;
            }
            __syncthreads();
            float o = 0.f;
            for (int j = 0; j < nk; j++) o = o + prob[ci][hd][j] * Vb[base + (size_t)(tok0 + j) * FE + tid];
            k.o = o;
            k.y = block_matvec128(wb + E::S_OW, wb + E::S_OB, o, tid, vec) + xq;
            k.zn = block_ln128_keep(k.y, k.zh, k.rstdm, wb + E::S_MG, wb + E::S_MB, tid, vec);
            k.z1 = block_matvec128(wb + E::S_W1, wb + E::S_B1, k.zn, tid, vec);
            k.g1 = gelu_erf(k.z1);
            ctx[FE * (1 + ci) + tid] = k.y + block_matvec128(wb + E::S_W2, wb + E::S_B2, k.g1, tid, vec);
            __syncthreads();
        }
        // the GMM head, forward: 64 wide, on wave 0
        float hcur = 0.f;
        if (tid < F) {
            hcur = blob[L.head_in_b + tid];
            for (int k = 0; k < E::CTX; k++) hcur = hcur + blob[L.head_in_w + k * F + tid] * ctx[k];
            pre[0][tid] = hcur;
            hcur = fmaxf(hcur, 0.f);
            for (int i = 0; i < a.head_layers; i++) {
                const float *__restrict__ w = blob + L.head_res + i * (W64 + F);
                hin[i][tid] = hcur;
                const float pr = matvec64(w, w + W64, hcur, tid);
                pre[1 + i][tid] = pr;
                hcur = hcur + fmaxf(pr, 0.f);
            }
            hin[a.head_layers][tid] = hcur;
        }
        __syncthreads();
        const int C = a.C, NO = 7 * C;
        if (tid < F)
            for (int o = tid; o < NO; o += 64) {
                float r = blob[L.head_b + o];
                for (int k = 0; k < F; k++) r = r + blob[L.head_w + k * NO + o] * hin[a.head_layers][k];
                raw[o] = r;
            }
        __syncthreads();
        // the rule's gradient, scaled by the row's upstream gradient
        if (tid < F) {
            auto load = [&](int k) { return raw[k]; };
            const float e[3] = {a.expert[(size_t)b * 3], a.expert[(size_t)b * 3 + 1], a.expert[(size_t)b * 3 + 2]};
            const bc_rule::Weights ws = bc_rule::weight_stats(C, load);
            const bc_grad_rule::Stats st = bc_grad_rule::stats(C, load, a.clip, ws, e);
            const float gn = a.gnll[b];
            for (int o = tid; o < NO; o += 64) draw[o] = bc_grad_rule::grad(C, load, a.clip, ws, e, st, o) * gn;
        }
        __syncthreads();
        if (tid < F) {
            // head.head, the residual block, and the gradient at head.input_layer's pre-activation (to vec)
            float dh = 0.f;
            for (int o = 0; o < NO; o++) {
                slice[L.head_w + o * F + tid] = slice[L.head_w + o * F + tid] + draw[o] * hcur;
                dh = dh + gb.WT[L.head_w + o * F + tid] * draw[o];
            }
            for (int o = tid; o < NO; o += 64) slice[L.head_b + o] = slice[L.head_b + o] + draw[o];
            for (int i = a.head_layers - 1; i >= 0; i--) {
                const int off = L.head_res + i * (W64 + F);
                const float dp = pre[1 + i][tid] > 0.f ? dh : 0.f;
                outer64(slice + off, slice + off + W64, dp, hin[i][tid], tid);
                dh = dh + matvec64_t(gb.WT + off, dp, tid);
            }
            const float dp = pre[0][tid] > 0.f ? dh : 0.f;
            slice[L.head_in_b + tid] = slice[L.head_in_b + tid] + dp;
            vec[tid] = dp;
        }
        __syncthreads();
        {
            // head.input_layer [64][384]: thread tid holds feature tid of each third of the context
            float dc[3] = {0.f, 0.f, 0.f};
            for (int o = 0; o < F; o++) {
                const float dpo = vec[o];
#pragma unroll
                for (int j = 0; j < 3; j++) {
                    const int at = L.head_in_w + o * E::CTX + FE * j + tid;
                    slice[at] = slice[at] + dpo * ctx[FE * j + tid];
                    dc[j] = dc[j] + gb.WT[at] * dpo;
                }
            }
#pragma unroll
            for (int j = 0; j < 3; j++) dctx[FE * j + tid] = dc[j];
        }
        __syncthreads();
        float dxq = dctx[tid];
#pragma unroll
        for (int ci = 0; ci < 2; ci++) {
            const CrossKeep &k = keep[ci];
            const int tok0 = ci ? d.A : 1, nk = ci ? ROADS : d.A - 1;
            const int cw = L.cross[ci], cb = cw + E::C_BODY;
            const float *__restrict__ wtb = gb.WT + cb;
            float *__restrict__ nb = slice + cb, *__restrict__ nw = slice + cw;
            const float dout = dctx[FE * (1 + ci) + tid];
            const float dz1 = block_linear128_back(nb + E::S_W2, nb + E::S_B2, wtb + E::S_W2, dout, k.g1, tid, vec) * gelu_erf_grad(k.z1);
            const float dzn = block_linear128_back(nb + E::S_W1, nb + E::S_B1, wtb + E::S_W1, dz1, k.zn, tid, vec);
            nb[E::S_MG + tid] = nb[E::S_MG + tid] + dzn * k.zh;
            nb[E::S_MB + tid] = nb[E::S_MB + tid] + dzn;
            const float dy = dout + block_ln128_back(dzn, k.zh, k.rstdm, blob[cb + E::S_MG + tid], tid, vec);
            const float dao = block_linear128_back(nb + E::S_OW, nb + E::S_OB, wtb + E::S_OW, dy, k.o, tid, vec);
            dxq = dxq + dy;
            // the one-query attention
            vec[tid] = dao;
            __syncthreads();
            for (int j = tid; j < nk; j += 128) {
                const float *__restrict__ vp = Vb + base + (size_t)(tok0 + j) * FE;
                for (int g = 0; g < 4; g++) {
                    float s = 0.f;
                    for (int c = 0; c < 32; c++) s = s + vec[32 * g + c] * vp[32 * g + c];
                    ds[g][j] = s;  // dP
                }
            }
            __syncthreads();
            for (int g = 2 * wv; g < 2 * wv + 2; g++) {
                float part = 0.f;
                for (int j = lane; j < nk; j += 64) part = part + prob[ci][g][j] * ds[g][j];
                const float D = wave_sum(part);
                for (int j = lane; j < nk; j += 64) {
                    const bool masked = token_mask(d, pm, rm, b, tok0 + j) != 0;
                    ds[g][j] = masked ? 0.f : prob[ci][g][j] * (ds[g][j] - D);  // a masked score receives nothing
                }
            }
            __syncthreads();
            float dq = 0.f;
            const float qv = qs[ci][tid];
            for (int j = 0; j < nk; j++) {
                const size_t at = base + (size_t)(tok0 + j) * FE + tid;
                const float dsj = ds[hd][j];
                gb.dQ[at] = prob[ci][hd][j] * dao;  // dV
                gb.dO[at] = dsj * qv;               // dK
                dq = dq + dsj * Kb[at];
            }
            dq = dq * E::QSCALE;
            const float dqn = block_linear128_back(nb + E::S_QW, nb + E::S_QB, wtb + E::S_QW, dq, k.qn, tid, vec);
            nw[E::C_QG + tid] = nw[E::C_QG + tid] + dqn * k.xhq;
            nw[E::C_QB + tid] = nw[E::C_QB + tid] + dqn;
            dxq = dxq + block_ln128_back(dqn, k.xhq, k.rstdq, blob[cw + E::C_QG + tid], tid, vec);
        }
        gb.dX[base + tid] = dxq;
    }
}

template <int T>
TList transposes(const gd_bc_policy &p, const BCLayout &L) {
    using E = BCEnc<T>;
    constexpr int FE = E::FE, W = E::W;
    TList tl{};
    auto add = [&](int off, int nin, int nout) { tl.off[tl.n] = off, tl.nin[tl.n] = nin, tl.nout[tl.n] = nout, tl.n++; };
    for (int e = 0; e < 3; e++)
        for (int i = 0; i < 3; i++) add(L.net_rest[e] + 3 * FE + i * (W + 3 * FE), 0, 0);
    for (int i = 0; i < p.fusion_layers + 2 * p.branch_layers; i++)
        for (int f : {E::S_QW, E::S_KW, E::S_VW, E::S_OW, E::S_W1, E::S_W2}) add(L.self0 + i * E::S_SIZE + f, 0, 0);
    for (int ci = 0; ci < 2; ci++) {
        const int cb = L.cross[ci] + E::C_BODY;
        add(cb + E::S_KW, 0, 0), add(cb + E::S_VW, 0, 0);
        for (int f : {E::S_QW, E::S_OW, E::S_W1, E::S_W2}) add(cb + f, FE, FE);
    }
    add(L.head_in_w, E::CTX, F);
    for (int i = 0; i < p.head_layers; i++) add(L.head_res + i * (W64 + F), F, F);
    add(L.head_w, F, 7 * p.n_components);
    return tl;
}

long long round64(long long v) { return (v + 63) / 64 * 64; }

// the whole call at width T: launch_bc_backward's arguments
template <int T>
void backward(const gd_bc_policy &p, const gd_bc_grad &g, hipStream_t st, const float *obs, const unsigned char *partner_mask,
              const unsigned char *road_mask, int n, const float *expert_actions, const float *grad_nll, float *nll, float *grad) {
    constexpr int FE = BCEnc<T>::FE;
    const int A = p.max_agents, R = p.num_stack, NL = p.fusion_layers + p.branch_layers, P = g.num_partials;
    const BCDims d = bc_dims(p);
    const BCLayout L = bc_layout<T>(R, p.fusion_layers + 2 * p.branch_layers, p.head_layers, p.n_components);
    const BCLayout N = bc_nat_layout<T>(R, p.fusion_layers + 2 * p.branch_layers, p.head_layers, p.n_components);
    const size_t per = (size_t)p.chunk_rows * d.L * FE;
    float *X = p.scratch, *Kb = p.scratch + per, *Vb = p.scratch + 2 * per;
    float *WT = g.scratch, *XS = WT + round64(p.blob_floats);
    GradBufs gb{};
    gb.blob = p.blob, gb.WT = WT, gb.partials = g.partials, gb.G = g.grad_floats, gb.nat_delta = N.self0 - L.self0;
    gb.O = XS + (size_t)NL * per, gb.dX = gb.O + per, gb.dO = gb.dX + per, gb.dQ = gb.dO + per, gb.Q = gb.dQ + per;
    gb.ML = gb.Q + per, gb.D = gb.ML + (size_t)p.chunk_rows * d.L * 8;
    const size_t pn = (size_t)P * (size_t)g.grad_floats;
    hipLaunchKernelGGL(k_bcg_zero, dim3((unsigned)std::min<size_t>((pn + 255) / 256, 4096)), dim3(256), 0, st, g.partials, pn);
    const TList tl = transposes<T>(p, L);
    hipLaunchKernelGGL(k_bcg_transpose<T>, dim3((unsigned)tl.n), dim3(64), 0, st, tl, p.blob, WT);
    auto copy = [&](const float *src, float *dst, size_t floats) {
        hipLaunchKernelGGL(k_bcg_copy, dim3((unsigned)std::min<size_t>((floats / 4 + 255) / 256, 4096)), dim3(256), 0, st,
                           reinterpret_cast<const f4 *>(src), reinterpret_cast<f4 *>(dst), floats / 4);
    };
    gd_bc_outputs out{};
    out.nll = nll;
    const Segs cross = bc_cross_segs<T>(p);
    for (int r0 = 0; r0 < n; r0 += p.chunk_rows) {
        const int rows = std::min(p.chunk_rows, n - r0);
        const size_t used = (size_t)rows * d.L * FE;
        const float *o = obs + (size_t)r0 * R * d.D;
        const unsigned char *pm = partner_mask + (size_t)r0 * R * (A - 1), *rm = road_mask + (size_t)r0 * R * ROADS;
        launch_bc_embed(p, FE, st, o, rows, X);
        for (int i = 0; i < NL; i++) {
            copy(X, XS + (size_t)i * per, used);
            launch_bc_self_layer(p, FE, st, pm, rm, rows, i, X, Kb, Vb, nullptr, nullptr);
        }
        launch_bc_cross_kv(p, FE, st, rows, X, Kb, Vb);
        if (nll) launch_bc_head(p, FE, st, partner_mask, road_mask, r0, rows, true, nullptr, nullptr, expert_actions, out, X, Kb, Vb);
        HeadGradArgs ha{p.head_layers, p.n_components, p.clip_value, expert_actions + (size_t)r0 * 3, grad_nll + r0};
        if constexpr (T == 2)
            hipLaunchKernelGGL(k_bcg_head, dim3((unsigned)P), dim3(64), 0, st, d, L, ha, rows, gb, pm, rm, X, Kb, Vb);
        else
            hipLaunchKernelGGL(k_bcg_head_block, dim3((unsigned)P), dim3(128), 0, st, d, L, ha, rows, gb, pm, rm, X, Kb, Vb);
        hipLaunchKernelGGL(k_bcg_kvx<T>, dim3((unsigned)P), dim3(64), 0, st, d, cross, rows, gb, X);
        for (int i = NL - 1; i >= 0; i--) {
            const float *xs = XS + (size_t)i * per;
            const Segs sg = bc_layer_segs<T>(p, i);
            copy(xs, X, used);
            launch_bc_self_layer(p, FE, st, pm, rm, rows, i, X, Kb, Vb, gb.O, gb.ML);
            hipLaunchKernelGGL(k_bcg_post<T>, dim3((unsigned)P), dim3(64), 0, st, d, sg, rows, gb, xs);
            hipLaunchKernelGGL(k_bcg_dq<T>, dim3((unsigned)P), dim3(64), 0, st, d, sg, rows, gb, xs, pm, rm, Kb, Vb);
            hipLaunchKernelGGL(k_bcg_dkv<T>, dim3((unsigned)P), dim3(64), 0, st, d, sg, rows, gb, xs, pm, rm, Kb, Vb);
        }
        hipLaunchKernelGGL(k_bcg_embed<T>, dim3((unsigned)P), dim3(64), 0, st, d, L, N, rows, gb, o);
    }
    hipLaunchKernelGGL(k_bcg_reduce, dim3((unsigned)((g.grad_floats + 255) / 256)), dim3(256), 0, st, g.partials, P, g.grad_floats, grad);
}

}  // namespace

long long bc_grad_floats(int dim, int num_stack, int fusion_layers, int branch_layers, int head_layers, int n_components) {
    const int n_self = fusion_layers + 2 * branch_layers;
    return dim == 128 ? bc_nat_layout<4>(num_stack, n_self, head_layers, n_components).total
                      : bc_nat_layout<2>(num_stack, n_self, head_layers, n_components).total;
}

// the one place that sizes gd_bc_grad.scratch: the transposed weights, XS of every self-attention launch, O, dX, dO, dQ, Q
// (a token row of `dim` floats each), ML (8) and D (4, padded to 8) per token of a chunk
long long bc_grad_scratch_floats(int dim, int max_agents, int chunk_rows, int fusion_layers, int branch_layers, long long blob_floats) {
    return round64(blob_floats) + (long long)chunk_rows * (max_agents + ROADS) * (dim * (fusion_layers + branch_layers + 5) + 16);
}

void launch_bc_backward(const gd_bc_policy &p, int dim, const gd_bc_grad &g, hipStream_t st, const float *obs,
                        const unsigned char *partner_mask, const unsigned char *road_mask, int n, const float *expert_actions,
                        const float *grad_nll, float *nll, float *grad) {
    if (dim == 128)
        backward<4>(p, g, st, obs, partner_mask, road_mask, n, expert_actions, grad_nll, nll, grad);
    else
        backward<2>(p, g, st, obs, partner_mask, road_mask, n, expert_actions, grad_nll, nll, grad);
}

}  // namespace gd

