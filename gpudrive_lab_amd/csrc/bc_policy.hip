// Device BC policy forward (gd_bc_forward, gd_bc_forward_dim and the entry points built on them): the reference's
// EarlyFusionAttnBCNet in eval mode (gpudrive/integrations/il/model/model.py, networks.py) on the tensors
// DeviceExpertDataset.batch() writes, float32 throughout, at network_dim 64 (the reference's default) and 128 (its sweep's:
// baselines/il/sweep.yaml, network_dim 128, head_dim 64, num_layer [4, 3]).  The kernels are templates on T = network_dim / 32
// (bc_tile.hpp); the GMM head behind head.input_layer is 64 wide at either.
// A token is the ego (1), a partner (A - 1) or a road point (200): L = A + 200 per sample, a token row is 32 T floats.  A wave
// holds 32 tokens TRANSPOSED, as policy.hip does: lane (c = lane & 31, h = lane >> 5) belongs to token c, and its T 16-register
// accumulators hold the features 32 t + acc(r, h) of that token.  A Linear is then 16 T^2 v_mfma_f32_32x32x2_f32 with the
// accumulator itself as the B operand (k-step (t, r) contracts the features F and F + 4), LayerNorm a sum over a lane's 16 T
// registers plus one swap of the lane halves, tanh / GELU elementwise.  Per chunk of gd_bc_policy.chunk_rows samples the
// launches are:
//   k_bc_embed   a wave per 32 tokens of one kind.  Layer 1 gathers the token's R rows straight from obs [B][R][D] (time is the
//                slow index inside a token: _unpack_obs's permute), then three more Linear -> LayerNorm -> tanh.  Owns X[b][token].
//   k_bc_kv      a wave per 32 tokens: K = Wk LN(x) + bk, V = Wv LN(x) + bv.  Owns K[b][token], V[b][token].
//   k_bc_attn    a wave per 32 queries of one (sample, segment): q = (Wq LN(x) + bq) * HC^-1/2 for the HC = 8 T channels of a
//                head (1 / 4; at 128 one multiplication by the float32 nearest to 32^-1/2), then per head a streamed softmax
//                over the segment's keys in tiles of 32, ascending: S^T = K Q^T is HC / 2 k-steps into one accumulator (the
//                scores never leave registers), running max and sum per query, P^T is the B operand of O^T += V^T P^T with no
//                lane movement.  At 64 a head is half of a tile's registers and rows 16 .. 31 of O^T repeat its channels; at
//                128 a head IS tile t = hd and the product fills all 32 rows.  A masked key's score is -FLT_MAX (not -inf),
//                keys past the segment's end do not exist.  Then o_proj + x, and the MLP (LN, Linear, erf GELU, Linear) + its
//                input: one launch holds the layer.  At 64 x stays in registers across the heads; at 128 it is read again for
//                the residual.  Owns X[b][its 32 tokens], rewritten in place (no other wave reads them: keys and values come
//                from K and V).  fusion_attn is one segment of L tokens; ro_attn and rg_attn are two segments of ONE launch.
//   k_bc_head    (64) a wave per sample, lane per feature, plain arithmetic as policy.hip's ego embedder (one query token has
//                no tile to fill): both cross attentions (their K / V come from k_bc_kv on the kv_norm'ed tokens), the context,
//                the GMM head, bc_rule.hpp and every output of the row.
//   k_bc_head_block  (128) the same for a workgroup of 128 threads, a thread per encoder feature, sums through LDS: the
//                384-wide context, the 64-wide GMM head on threads 0 .. 63.
// 2 F + 2 S + 3 launches per chunk for F fusion and S branch layers.  Every sum has one owner and a fixed order; no atomics; no
// host synchronisation; every byte of every output given is stored on every call.  Masks are read with byte loads (their rows
// have odd pitch).  An MFMA is a chain of fmaf in k order with one rounding per product; everything else rounds every operation.
// The backward (bc_grad.hip, at either width) reruns these kernels per chunk through launch_bc_embed, launch_bc_self_layer,
// launch_bc_cross_kv and launch_bc_head; its SAVE instantiation of the attention kernel also stores the attention output
// before o_proj and the softmax's row statistics.
// The forward on a row list (gd_bc_forward_rows, launch_bc_forward_rows) is the same launches on the kernels' list
// instantiations (the pack of their last parameters is one BCRows).  A list position q belongs to chunk q / chunk_rows and to
// scratch slot q % chunk_rows; the workgroup of a slot loads the list's length, returns if its position is past it (or its
// entry is no row) before it loads, stores to LDS or synchronises anything else, and otherwise computes row rows[q]: X / K / V
// by slot; obs, the masks, u, z, expert_actions and every output by the row.  No result of a sample depends on the samples
// beside it, so a listed row gets the full forward's bits.  The host knows no length: every chunk is launched.
// The 128-wide kernels were first written out as a second file beside the 64-wide ones; both are now instantiations of one
// text, and each compiles to the machine code it had as a file of its own.
#include "bc_tile.hpp"

namespace gd {

namespace {

// ---- token embedding

// grid (1 + ceil((A - 1) / 32) + 7, rows): tile 0 is the ego, then the partner tiles, then the road tiles.  List = (BCRows): obs
// is the whole call's, X is indexed by slot
template <int T, class... List>
__global__ __launch_bounds__(64) void k_bc_embed(BCDims d, BCLayout L, const float *__restrict__ blob, const float *__restrict__ obs,
                                                 float *__restrict__ X, List... lr) {
    constexpr int FE = BCEnc<T>::FE, W = BCEnc<T>::W;
    const int lane = threadIdx.x, h = lane >> 5, col = lane & 31;
    const int slot = blockIdx.y, tile = blockIdx.x;
    const int b = bc_sample(slot, lr...);
    if constexpr (sizeof...(List) > 0) {
        if (b < 0) return;
    }
    const int ptiles = (d.A - 1 + 31) / 32;
    const int kind = tile == 0 ? 0 : tile <= ptiles ? 1 : 2;
    const int count = kind == 0 ? 1 : kind == 1 ? d.A - 1 : ROADS;
    const int e = (kind == 0 ? 0 : kind == 1 ? (tile - 1) * 32 : (tile - 1 - ptiles) * 32) + col;
    const bool live = e < count;
    const int ec = live ? e : count - 1;  // a lane past the end computes the last token again and stores nothing
    const float *__restrict__ x = obs + (size_t)b * d.R * d.D;
    const float *__restrict__ w0 = blob + L.net_w0[kind];
    const float *__restrict__ rest = blob + L.net_rest[kind];
    f16v a[T], o[T];
    if (kind == 2)
        embed_first<ROAD_K>(x, d.D, d.R, EGO_K + PARTNER_K * (d.A - 1), ec, w0, rest, a, lane, h);
    else
        embed_first<PARTNER_K>(x, d.D, d.R, kind == 0 ? 0 : EGO_K, ec, w0, rest, a, lane, h);
    layer_norm(a, rest + FE, rest + 2 * FE, h);
#pragma unroll
    for (int t = 0; t < T; t++)
#pragma unroll
        for (int r = 0; r < 16; r++) a[t][r] = tanhf(a[t][r]);
    for (int i = 0; i < 3; i++) {
        const float *__restrict__ w = rest + 3 * FE + i * (W + 3 * FE);
        linear(a, w, w + W, o, lane, h);
        layer_norm(o, w + W + FE, w + W + 2 * FE, h);
#pragma unroll
        for (int t = 0; t < T; t++)
#pragma unroll
            for (int r = 0; r < 16; r++) a[t][r] = tanhf(o[t][r]);
    }
    const int tok = (kind == 0 ? 0 : kind == 1 ? 1 : d.A) + e;
    if (live) store_tok(X + ((size_t)slot * d.L + tok) * FE, a, h);
}

// ---- attention

// grid (sum of tiles, rows).  Reads and writes the scratch only: b is the slot, List = (BCRows) says which slots hold a sample
template <int T, class... List>
__global__ __launch_bounds__(64) void k_bc_kv(BCDims d, Segs sg, const float *__restrict__ blob, const float *__restrict__ X,
                                              float *__restrict__ Kb, float *__restrict__ Vb, List... lr) {
    const int lane = threadIdx.x, h = lane >> 5, col = lane & 31;
    const int b = blockIdx.y;
    if constexpr (sizeof...(List) > 0) {
        if (bc_sample(b, lr...) < 0) return;
    }
    int tile = blockIdx.x;
    const bool second = tile >= sg.s[0].tiles;
    const Seg &s = sg.s[second ? 1 : 0];
    if (second) tile -= sg.s[0].tiles;
    const int j = tile * 32 + col;
    const bool live = j < s.ntok;
    const size_t at = ((size_t)b * d.L + s.tok0 + (live ? j : s.ntok - 1)) * BCEnc<T>::FE;
    f16v x[T], o[T];
    load_tok(X + at, x, h);
    layer_norm(x, blob + s.ng, blob + s.nb, h);
    linear(x, blob + s.kw, blob + s.kb, o, lane, h);
    if (live) store_tok(Kb + at, o, h);
    linear(x, blob + s.vw, blob + s.vb, o, lane, h);
    if (live) store_tok(Vb + at, o, h);
}

__device__ __forceinline__ float *bc_save_o(float *osave, float *) { return osave; }
__device__ __forceinline__ float *bc_save_ml(float *, float *ml) { return ml; }

// grid (sum of tiles, rows).  Save = (float *osave, float *ml): also store the attention output before o_proj (osave
// [b][token][32 T]) and per (token, head) the softmax's final running max and its sum (ml [b][token][8]: m of the four heads,
// then the four sums), for the backward.  Save = (BCRows): the forward on a row list, the masks are the whole call's, X / K / V
// are indexed by slot
template <int T, class... Save>
__global__ __launch_bounds__(64) void k_bc_attn(BCDims d, Segs sg, const float *__restrict__ blob,
                                                const unsigned char *__restrict__ pm, const unsigned char *__restrict__ rm,
                                                float *__restrict__ X, const float *__restrict__ Kb, const float *__restrict__ Vb,
                                                Save... save) {
    using E = BCEnc<T>;
    constexpr int FE = E::FE, HC = E::HC;
    constexpr bool SAVE = sizeof...(Save) == 2, LIST = sizeof...(Save) == 1;
    constexpr bool KEEP_X = T == 2;  // a register-pressure decision: at 128 the layer's input is read again for the residual
    __shared__ unsigned char msk[MAX_TOKENS];
    const int lane = threadIdx.x, h = lane >> 5, col = lane & 31;
    const int slot = blockIdx.y;
    int b = slot;
    if constexpr (LIST) {
        b = bc_sample(slot, save...);
        if (b < 0) return;
    }
    int tile = blockIdx.x;
    const bool second = tile >= sg.s[0].tiles;
    const Seg &s = sg.s[second ? 1 : 0];
    if (second) tile -= sg.s[0].tiles;
    const int ntok = s.ntok;
    for (int j = lane; j < ntok; j += 64) msk[j] = token_mask(d, pm, rm, b, s.tok0 + j);
    __syncthreads();
    const float *__restrict__ w = blob + s.w;
    const int qi = tile * 32 + col;
    const bool live = qi < ntok;
    const size_t seg_at = ((size_t)slot * d.L + s.tok0) * FE;
    float *__restrict__ xrow = X + seg_at + (size_t)(live ? qi : ntok - 1) * FE;
    f16v x[T], q[T], o[T];
    {
        f16v hn[T];
        load_tok(xrow, hn, h);
        if constexpr (KEEP_X) __builtin_memcpy(x, hn, sizeof(x));  // as one block: a copy per tile compiles to other code
        layer_norm(hn, w + E::S_NG, w + E::S_NB, h);
        linear(hn, w + E::S_QW, w + E::S_QB, q, lane, h);
    }
#pragma unroll
    for (int t = 0; t < T; t++)
#pragma unroll
        for (int r = 0; r < 16; r++) q[t][r] = q[t][r] * E::QSCALE;

#pragma unroll
    for (int hd = 0; hd < 4; hd++) {
        const int t = hd * HC / 32, rb = (hd * HC % 32) / 2;  // the head's HC channels are registers rb .. rb + HC / 2 - 1 of tile t
        float m = -INFINITY, l = 0.f;
        f16v O;
#pragma unroll
        for (int r = 0; r < 16; r++) O[r] = 0.f;
        for (int kb = 0; kb < ntok; kb += 32) {
            const int key = min(kb + col, ntok - 1);
            const float *__restrict__ kp = Kb + seg_at + (size_t)key * FE + HC * hd + 4 * h;
            f4 kv[HC / 8];
#pragma unroll
            for (int g = 0; g < HC / 8; g++) kv[g] = *reinterpret_cast<const f4 *>(kp + 8 * g);
            f16v sc;
#pragma unroll
            for (int r = 0; r < 16; r++) sc[r] = 0.f;
            // S^T[key][query]: k-step r contracts the channels HC hd + acc_row(r, 0) and + 4
#pragma unroll
            for (int r = 0; r < HC / 2; r++) sc = __builtin_amdgcn_mfma_f32_32x32x2f32(kv[r >> 2][r & 3], q[t][rb + r], sc, 0, 0, 0);
            float tm = -INFINITY;
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int kk = kb + acc_row(r, h);
                if (kk < ntok) {
                    if (msk[kk]) sc[r] = -FLT_MAX;
                    tm = fmaxf(tm, sc[r]);
                }
            }
            tm = fmaxf(tm, __shfl_xor(tm, 32));
            const float mn = fmaxf(m, tm);  // finite: the first tile always holds a key
            const float scale = expf(m - mn);
            float ps = 0.f;
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int kk = kb + acc_row(r, h);
                const float p = kk < ntok ? expf(sc[r] - mn) : 0.f;
                sc[r] = p;
                ps = ps + p;
            }
            l = l * scale + ps;
#pragma unroll
            for (int r = 0; r < 16; r++) O[r] = O[r] * scale;
            // O^T[channel][query] += V^T P^T: P's registers are the B operand as they are; lane c supplies channel HC hd + c, at
            // 64 rows 16 .. 31 repeat the channels
            const float *__restrict__ vp = Vb + seg_at + HC * hd + (col & (HC - 1));
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int vk = min(kb + acc_row(r, h), ntok - 1);
                O = __builtin_amdgcn_mfma_f32_32x32x2f32(vp[(size_t)vk * FE], sc[r], O, 0, 0, 0);
            }
            m = mn;
        }
        const float lt = l + __shfl_xor(l, 32);
#pragma unroll
        for (int r = 0; r < HC / 2; r++) o[t][rb + r] = O[r] / lt;
        if constexpr (SAVE) {
            if (live && h == 0) {
                float *__restrict__ st = bc_save_ml(save...) + ((size_t)b * d.L + s.tok0 + qi) * 8;
                st[hd] = m, st[4 + hd] = lt;
            }
        }
    }
    if constexpr (SAVE) {
        if (live) store_tok(bc_save_o(save...) + seg_at + (size_t)qi * FE, o, h);
    }

    f16v y[T], z[T], z1[T];
    linear(o, w + E::S_OW, w + E::S_OB, y, lane, h);
    if constexpr (!KEEP_X) load_tok(xrow, x, h);  // nobody else writes these rows
#pragma unroll
    for (int t = 0; t < T; t++)
#pragma unroll
        for (int r = 0; r < 16; r++) {
            y[t][r] = y[t][r] + x[t][r];
            z[t][r] = y[t][r];
        }
    layer_norm(z, w + E::S_MG, w + E::S_MB, h);
    linear(z, w + E::S_W1, w + E::S_B1, z1, lane, h);
#pragma unroll
    for (int t = 0; t < T; t++)
#pragma unroll
        for (int r = 0; r < 16; r++) z1[t][r] = gelu_erf(z1[t][r]);
    linear(z1, w + E::S_W2, w + E::S_B2, z, lane, h);
#pragma unroll
    for (int t = 0; t < T; t++)
#pragma unroll
        for (int r = 0; r < 16; r++) y[t][r] = y[t][r] + z[t][r];
    if (live) store_tok(xrow, y, h);
}

// ---- cross attention, context, head, rule: one query token per sample, a thread per encoder feature

// network_dim 64: a wave per sample, sums by shuffles.  grid (rows).  List = (BCRows): the masks and every pointer of `a` are the
// whole call's, X / K / V are indexed by slot
template <class... List>
__global__ __launch_bounds__(64) void k_bc_head(BCDims d, BCLayout L, BCHeadArgs a, const float *__restrict__ blob,
                                                const unsigned char *__restrict__ pm, const unsigned char *__restrict__ rm,
                                                const float *__restrict__ X, const float *__restrict__ Kb,
                                                const float *__restrict__ Vb, List... lr) {
    using E = BCEnc<2>;
    __shared__ float sc[4][ROADS];
    __shared__ float ctx[E::CTX];
    __shared__ float vec[F];
    __shared__ float raw[MAX_HEAD_OUT];
    const int lane = threadIdx.x, slot = blockIdx.x, hd = lane >> 4;
    const int b = bc_sample(slot, lr...);
    if constexpr (sizeof...(List) > 0) {
        if (b < 0) return;
    }
    const size_t base = (size_t)slot * d.L * F;
    const float xq = X[base + lane];  // ro_attn's token 0: the query of both cross attentions and the context's first third
    ctx[lane] = xq;
    for (int ci = 0; ci < 2; ci++) {
        const int tok0 = ci ? d.A : 1, nk = ci ? ROADS : d.A - 1;
        const float *__restrict__ w = blob + L.cross[ci];
        const float *__restrict__ wb = w + E::C_BODY;  // the fields S_* of a self layer follow the two norms
        const float qn = wave_ln(xq, w + E::C_QG, w + E::C_QB, lane);
        vec[lane] = matvec64(wb + E::S_QW, wb + E::S_QB, qn, lane) * E::QSCALE;
        __syncthreads();
        for (int j = lane; j < nk; j += 64) {
            const float *__restrict__ kp = Kb + base + (size_t)(tok0 + j) * F;
            const bool masked = token_mask(d, pm, rm, b, tok0 + j) != 0;
            for (int g = 0; g < 4; g++) {
                float s = 0.f;
                for (int c = 0; c < 16; c++) s = s + vec[16 * g + c] * kp[16 * g + c];
                sc[g][j] = masked ? -FLT_MAX : s;
            }
        }
        __syncthreads();
        for (int g = 0; g < 4; g++) {
            float m = -INFINITY;
            for (int j = lane; j < nk; j += 64) m = fmaxf(m, sc[g][j]);
            m = wave_max(m);
            float ps = 0.f;
            for (int j = lane; j < nk; j += 64) {
                const float p = expf(sc[g][j] - m);
                sc[g][j] = p;
                ps = ps + p;
            }
            const float S = wave_sum(ps);
            for (int j = lane; j < nk; j += 64) sc[g][j] = sc[g][j] / S;
            if (ci == 0 && a.ego_attn_score) {  // the row divided by its own sum, as get_context returns it
                float ts = 0.f;
                for (int j = lane; j < nk; j += 64) ts = ts + sc[g][j];
                const float T = wave_sum(ts);
                for (int j = lane; j < nk; j += 64) a.ego_attn_score[((size_t)b * 4 + g) * nk + j] = sc[g][j] / T;
            }
        }
        __syncthreads();
        float o = 0.f;
        for (int j = 0; j < nk; j++) o = o + sc[hd][j] * Vb[base + (size_t)(tok0 + j) * F + lane];
        const float y = matvec64(wb + E::S_OW, wb + E::S_OB, o, lane) + xq;
        float zz = wave_ln(y, wb + E::S_MG, wb + E::S_MB, lane);
        zz = gelu_erf(matvec64(wb + E::S_W1, wb + E::S_B1, zz, lane));
        zz = matvec64(wb + E::S_W2, wb + E::S_B2, zz, lane);
        ctx[F * (1 + ci) + lane] = y + zz;
        __syncthreads();
    }
    // the GMM head
    float hcur = blob[L.head_in_b + lane];
    for (int k = 0; k < E::CTX; k++) hcur = hcur + blob[L.head_in_w + k * F + lane] * ctx[k];
    hcur = fmaxf(hcur, 0.f);
    for (int i = 0; i < a.head_layers; i++) {
        const float *__restrict__ w = blob + L.head_res + i * (W64 + F);
        hcur = hcur + fmaxf(matvec64(w, w + W64, hcur, lane), 0.f);
    }
    vec[lane] = hcur;
    __syncthreads();
    const int C = a.C, NO = 7 * C;
    for (int o = lane; o < NO; o += 64) {
        float r = blob[L.head_b + o];
        for (int k = 0; k < F; k++) r = r + blob[L.head_w + k * NO + o] * vec[k];
        raw[o] = r;
    }
    __syncthreads();
    auto load = [&](int k) { return raw[k]; };
    const bc_rule::Weights ws = bc_rule::weight_stats(C, load);
    if (a.context)
        for (int i = lane; i < E::CTX; i += 64) a.context[(size_t)b * E::CTX + i] = ctx[i];
    for (int i = lane; i < 3 * C; i += 64) {
        const float lc = bc_rule::logcov(C, load, a.clip, i);
        if (a.means) a.means[(size_t)b * 3 * C + i] = raw[i];
        if (a.logcov) a.logcov[(size_t)b * 3 * C + i] = lc;
        if (a.cov) a.cov[(size_t)b * 3 * C + i] = expf(lc);
    }
    if (a.weights && lane < C) a.weights[(size_t)b * C + lane] = bc_rule::weight(C, load, ws, lane);
    if (lane == 0) {
        const int c = a.deterministic ? bc_rule::mode(C, load, ws) : bc_rule::pick(C, load, ws, a.u[b]);
        if (a.component) a.component[b] = c;
        if (a.actions)
            for (int k = 0; k < 3; k++)
                a.actions[(size_t)b * 3 + k] = a.deterministic ? raw[3 * c + k] : bc_rule::sampled(C, load, a.clip, c, k, a.z[(size_t)b * 3 + k]);
        if (a.nll) {
            const float e[3] = {a.expert[(size_t)b * 3], a.expert[(size_t)b * 3 + 1], a.expert[(size_t)b * 3 + 2]};
            a.nll[b] = bc_rule::nll(C, load, a.clip, ws, e);
        }
    }
}

// network_dim 128: a workgroup of 128 threads per sample, sums through LDS (block_ln128, block_matvec128).  grid (rows).
// List = (BCRows): as for k_bc_head.  The softmax over sc[g][j] and everything from raw[] onward are k_bc_head's text with the
// thread count and the context's width changed.  They are written out twice on purpose: as a shared __forceinline__ function
// (raw and ctx as pointers, as array references, or raw through the caller's lambda; the widths as arguments or as template
// parameters) both kernels compile to other code than they had -- registers renamed from the softmax loop on, the context
// loop's guard folded differently -- and this file's rule is that a kernel keeps its machine code (NOTEBOOK.md has the counts)
template <class... List>
__global__ __launch_bounds__(128) void k_bc_head_block(BCDims d, BCLayout L, BCHeadArgs a, const float *__restrict__ blob,
                                                       const unsigned char *__restrict__ pm, const unsigned char *__restrict__ rm,
                                                       const float *__restrict__ X, const float *__restrict__ Kb,
                                                       const float *__restrict__ Vb, List... lr) {
    using E = BCEnc<4>;
    constexpr int FE = E::FE;
    __shared__ float sc[4][ROADS];
    __shared__ float ctx[E::CTX];
    __shared__ float vec[FE];
    __shared__ float raw[MAX_HEAD_OUT];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, slot = blockIdx.x, hd = tid >> 5;
    const int b = bc_sample(slot, lr...);
    if constexpr (sizeof...(List) > 0) {
        if (b < 0) return;
    }
    const size_t base = (size_t)slot * d.L * FE;
    const float xq = X[base + tid];  // ro_attn's token 0: the query of both cross attentions and the context's first third
    ctx[tid] = xq;
    for (int ci = 0; ci < 2; ci++) {
        const int tok0 = ci ? d.A : 1, nk = ci ? ROADS : d.A - 1;
        const float *__restrict__ w = blob + L.cross[ci];
        const float *__restrict__ wb = w + E::C_BODY;  // the fields S_* of a self layer follow the two norms
        const float qn = block_ln128(xq, w + E::C_QG, w + E::C_QB, tid, vec);
        const float qv = block_matvec128(wb + E::S_QW, wb + E::S_QB, qn, tid, vec) * E::QSCALE;
        vec[tid] = qv;
        __syncthreads();
        for (int j = tid; j < nk; j += 128) {
            const float *__restrict__ kp = Kb + base + (size_t)(tok0 + j) * FE;
            const bool masked = token_mask(d, pm, rm, b, tok0 + j) != 0;
            for (int g = 0; g < 4; g++) {
                float s = 0.f;
                for (int c = 0; c < 32; c++) s = s + vec[32 * g + c] * kp[32 * g + c];
                sc[g][j] = masked ? -FLT_MAX : s;
            }
        }
        __syncthreads();
        for (int g = 2 * wv; g < 2 * wv + 2; g++) {  // a wave per two heads, its lanes stride the keys
            float m = -INFINITY;
            for (int j = lane; j < nk; j += 64) m = fmaxf(m, sc[g][j]);
            m = wave_max(m);
            float ps = 0.f;
            for (int j = lane; j < nk; j += 64) {
                const float p = expf(sc[g][j] - m);
                sc[g][j] = p;
                ps = ps + p;
            }
            const float S = wave_sum(ps);
            for (int j = lane; j < nk; j += 64) sc[g][j] = sc[g][j] / S;
            if (ci == 0 && a.ego_attn_score) {  // the row divided by its own sum, as get_context returns it
                float ts = 0.f;
                for (int j = lane; j < nk; j += 64) ts = ts + sc[g][j];
                const float T = wave_sum(ts);
                for (int j = lane; j < nk; j += 64) a.ego_attn_score[((size_t)b * 4 + g) * nk + j] = sc[g][j] / T;
            }
        }
        __syncthreads();
        float o = 0.f;
        for (int j = 0; j < nk; j++) o = o + sc[hd][j] * Vb[base + (size_t)(tok0 + j) * FE + tid];
        const float y = block_matvec128(wb + E::S_OW, wb + E::S_OB, o, tid, vec) + xq;
        float zz = block_ln128(y, wb + E::S_MG, wb + E::S_MB, tid, vec);
        zz = gelu_erf(block_matvec128(wb + E::S_W1, wb + E::S_B1, zz, tid, vec));
        zz = block_matvec128(wb + E::S_W2, wb + E::S_B2, zz, tid, vec);
        ctx[FE * (1 + ci) + tid] = y + zz;
        __syncthreads();
    }
    // the GMM head, 64 wide: threads 0 .. 63 hold a feature each
    float hcur = 0.f;
    if (tid < F) {
        hcur = blob[L.head_in_b + tid];
        for (int k = 0; k < E::CTX; k++) hcur = hcur + blob[L.head_in_w + k * F + tid] * ctx[k];
        hcur = fmaxf(hcur, 0.f);
    }
    for (int i = 0; i < a.head_layers; i++) {
        const float *__restrict__ w = blob + L.head_res + i * (W64 + F);
        if (tid < F) vec[tid] = hcur;
        __syncthreads();
        if (tid < F) {
            float o = w[W64 + tid];
            for (int k = 0; k < F; k++) o = o + w[k * F + tid] * vec[k];
            hcur = hcur + fmaxf(o, 0.f);
        }
        __syncthreads();
    }
    if (tid < F) vec[tid] = hcur;
    __syncthreads();
    const int C = a.C, NO = 7 * C;
    for (int o = tid; o < NO; o += 128) {
        float r = blob[L.head_b + o];
        for (int k = 0; k < F; k++) r = r + blob[L.head_w + k * NO + o] * vec[k];
        raw[o] = r;
    }
    __syncthreads();
    auto load = [&](int k) { return raw[k]; };
    const bc_rule::Weights ws = bc_rule::weight_stats(C, load);
    if (a.context)
        for (int i = tid; i < E::CTX; i += 128) a.context[(size_t)b * E::CTX + i] = ctx[i];
    for (int i = tid; i < 3 * C; i += 128) {
        const float lc = bc_rule::logcov(C, load, a.clip, i);
        if (a.means) a.means[(size_t)b * 3 * C + i] = raw[i];
        if (a.logcov) a.logcov[(size_t)b * 3 * C + i] = lc;
        if (a.cov) a.cov[(size_t)b * 3 * C + i] = expf(lc);
    }
    if (a.weights && tid < C) a.weights[(size_t)b * C + tid] = bc_rule::weight(C, load, ws, tid);
    if (tid == 0) {
        const int c = a.deterministic ? bc_rule::mode(C, load, ws) : bc_rule::pick(C, load, ws, a.u[b]);
        if (a.component) a.component[b] = c;
        if (a.actions)
            for (int k = 0; k < 3; k++)
                a.actions[(size_t)b * 3 + k] = a.deterministic ? raw[3 * c + k] : bc_rule::sampled(C, load, a.clip, c, k, a.z[(size_t)b * 3 + k]);
        if (a.nll) {
            const float e[3] = {a.expert[(size_t)b * 3], a.expert[(size_t)b * 3 + 1], a.expert[(size_t)b * 3 + 2]};
            a.nll[b] = bc_rule::nll(C, load, a.clip, ws, e);
        }
    }
}

// evaluate()'s running sums: one wave; lane i sums the rows i, i + 64, .. in ascending order, then one fixed tree.
// acc[0] += mean nll; acc[1..3] += mean |pred - expert| per dimension; acc[4..6] += the sums of |pred - expert| where the
// expert's magnitude exceeds thr[k]; acc[7..9] += their counts; acc[10] += 1 (batches)
__global__ __launch_bounds__(64) void k_bc_eval_acc(int n, const float *__restrict__ nll, const float *__restrict__ pred,
                                                    const float *__restrict__ expert, float *__restrict__ acc) {
    const int lane = threadIdx.x;
    const float thr[3] = {2.f, 0.035f, 0.023f};
    float v[10];
    for (int i = 0; i < 10; i++) v[i] = 0.f;
    for (int r = lane; r < n; r += 64) {
        v[0] = v[0] + nll[r];
        for (int k = 0; k < 3; k++) {
            const float e = expert[(size_t)r * 3 + k], dlt = fabsf(pred[(size_t)r * 3 + k] - e);
            v[1 + k] = v[1 + k] + dlt;
            if (fabsf(e) > thr[k]) v[4 + k] = v[4 + k] + dlt, v[7 + k] = v[7 + k] + 1.f;
        }
    }
    for (int i = 0; i < 10; i++) v[i] = wave_sum(v[i]);
    if (lane == 0) {
        for (int i = 0; i < 4; i++) acc[i] = acc[i] + v[i] / (float)n;
        for (int i = 4; i < 10; i++) acc[i] = acc[i] + v[i];
        acc[10] = acc[10] + 1.f;
    }
}

// ---- the host: one launch each, at width T, of the whole rows of a chunk (no pack) or of a row list's (List = BCRows)

template <int T, class... List>
void embed(const gd_bc_policy &p, hipStream_t st, const float *obs, unsigned slots, float *X, List... lr) {
    const unsigned etiles = (unsigned)(1 + (p.max_agents - 1 + 31) / 32 + (ROADS + 31) / 32);
    hipLaunchKernelGGL((k_bc_embed<T, List...>), dim3(etiles, slots), dim3(64), 0, st, bc_dims(p), bc_layout<T>(p), p.blob, obs, X, lr...);
}

inline dim3 seg_grid(const Segs &sg, unsigned slots) {
    unsigned tiles = 0;
    for (int i = 0; i < sg.n; i++) tiles += (unsigned)sg.s[i].tiles;
    return dim3(tiles, slots);
}

template <int T, class... List>
void kv(const gd_bc_policy &p, hipStream_t st, const Segs &sg, unsigned slots, const float *X, float *Kb, float *Vb, List... lr) {
    hipLaunchKernelGGL((k_bc_kv<T, List...>), seg_grid(sg, slots), dim3(64), 0, st, bc_dims(p), sg, p.blob, X, Kb, Vb, lr...);
}

template <int T, class... Save>
void attn(const gd_bc_policy &p, hipStream_t st, const Segs &sg, const unsigned char *pm, const unsigned char *rm, unsigned slots,
          float *X, const float *Kb, const float *Vb, Save... save) {
    hipLaunchKernelGGL((k_bc_attn<T, Save...>), seg_grid(sg, slots), dim3(64), 0, st, bc_dims(p), sg, p.blob, pm, rm, X, Kb, Vb, save...);
}

template <int T, class... List>
void head(const gd_bc_policy &p, hipStream_t st, const unsigned char *pm, const unsigned char *rm, unsigned slots, const BCHeadArgs &a,
          const float *X, const float *Kb, const float *Vb, List... lr) {
    if constexpr (T == 2)
        hipLaunchKernelGGL(k_bc_head<List...>, dim3(slots), dim3(64), 0, st, bc_dims(p), bc_layout<T>(p), a, p.blob, pm, rm, X, Kb, Vb, lr...);
    else
        hipLaunchKernelGGL(k_bc_head_block<List...>, dim3(slots), dim3(128), 0, st, bc_dims(p), bc_layout<T>(p), a, p.blob, pm, rm, X, Kb,
                           Vb, lr...);
}

// the head kernel's arguments for the whole call's rows
BCHeadArgs head_args(const gd_bc_policy &p, bool deterministic, const float *u, const float *z, const float *expert_actions,
                     const gd_bc_outputs &out) {
    BCHeadArgs a{};
    a.head_layers = p.head_layers, a.C = p.n_components, a.deterministic = deterministic ? 1 : 0, a.clip = p.clip_value;
    a.u = u, a.z = z, a.expert = expert_actions;
    a.context = out.context, a.means = out.means, a.logcov = out.log_covariances, a.cov = out.covariances;
    a.weights = out.weights, a.actions = out.actions, a.nll = out.nll, a.ego_attn_score = out.ego_attn_score;
    a.component = out.component;
    return a;
}

// ... and for the rows r0 .. of it: every pointer that is given, advanced by r0 of its rows
BCHeadArgs offset(BCHeadArgs a, int r0, int A, int ctxw) {
    auto adv = [r0](auto *&ptr, size_t per_row) { if (ptr) ptr += r0 * per_row; };
    const size_t C = (size_t)a.C;
    adv(a.u, 1), adv(a.z, 3), adv(a.expert, 3);
    adv(a.context, ctxw), adv(a.means, 3 * C), adv(a.logcov, 3 * C), adv(a.cov, 3 * C), adv(a.weights, C), adv(a.actions, 3);
    adv(a.nll, 1), adv(a.ego_attn_score, 4 * (size_t)(A - 1)), adv(a.component, 1);
    return a;
}

// The probe read-outs of a chunk (bc_readout.hip), right after self layer `at` (-1: none).  They read 64-wide tokens: there
// is none at 128.  Without a list the chunk is the rows r0 .. and the kernel drops the rows whose byte of `dead` is set
struct ReadOut {
    const gd_bc_readout *ro;
    const unsigned char *dead;
    int at, r0, n;
};
void read_out(const gd_bc_policy &p, hipStream_t st, const ReadOut &rd, unsigned slots, const float *X) {
    launch_bc_readout(p, st, *rd.ro, rd.dead, rd.r0, (int)slots, X, nullptr, nullptr, rd.n);
}
void read_out(const gd_bc_policy &p, hipStream_t st, const ReadOut &rd, unsigned slots, const float *X, const BCRows &lr) {
    launch_bc_readout(p, st, *rd.ro, nullptr, lr.q0, (int)slots, X, lr.rows, lr.count, lr.n);
}

// one chunk: the slots' samples are the rows obs, the masks and `a` start at (List empty) or the list's, obs, the masks and `a`
// being the whole call's (List = BCRows)
template <int T, class... List>
void launch_chunk(const gd_bc_policy &p, hipStream_t st, const float *obs, const unsigned char *pm, const unsigned char *rm,
                  unsigned slots, const BCHeadArgs &a, const ReadOut &rd, List... lr) {
    const size_t per = (size_t)p.chunk_rows * (p.max_agents + ROADS) * BCEnc<T>::FE;
    float *X = p.scratch, *Kb = p.scratch + per, *Vb = p.scratch + 2 * per;
    embed<T>(p, st, obs, slots, X, lr...);
    for (int i = 0; i < p.fusion_layers + p.branch_layers; i++) {
        const Segs sg = bc_layer_segs<T>(p, i);
        kv<T>(p, st, sg, slots, X, Kb, Vb, lr...);
        attn<T>(p, st, sg, pm, rm, slots, X, Kb, Vb, lr...);
        if constexpr (T == 2) {
            if (i == rd.at) read_out(p, st, rd, slots, X, lr...);
        }
    }
    kv<T>(p, st, bc_cross_segs<T>(p), slots, X, Kb, Vb, lr...);
    head<T>(p, st, pm, rm, slots, a, X, Kb, Vb, lr...);
}

template <int T>
void forward(const gd_bc_policy &p, hipStream_t st, const float *obs, const unsigned char *partner_mask, const unsigned char *road_mask,
             int n, const BCHeadArgs &a, const gd_bc_readout *readout, const unsigned char *dead) {
    const BCDims d = bc_dims(p);
    const int read_at = readout ? bc_tap_layer(p, readout->tap, readout->layer) : -1;
    for (int r0 = 0; r0 < n; r0 += p.chunk_rows)
        launch_chunk<T>(p, st, obs + (size_t)r0 * d.R * d.D, partner_mask + (size_t)r0 * d.R * (d.A - 1),
                        road_mask + (size_t)r0 * d.R * ROADS, (unsigned)std::min(p.chunk_rows, n - r0), offset(a, r0, d.A, BCEnc<T>::CTX),
                        ReadOut{readout, dead, read_at, r0, n});
}

// every chunk of list positions with the full forward's grids -- the host does not know the list's length -- on the list
// instantiations; a chunk past the list is workgroups that return at their first load
template <int T>
void forward_rows(const gd_bc_policy &p, hipStream_t st, const float *obs, const unsigned char *partner_mask,
                  const unsigned char *road_mask, int n, const BCHeadArgs &a, const int32_t *rows, const int32_t *count,
                  const gd_bc_readout *readout) {
    const int read_at = readout ? bc_tap_layer(p, readout->tap, readout->layer) : -1;
    for (int q0 = 0; q0 < n; q0 += p.chunk_rows)
        launch_chunk<T>(p, st, obs, partner_mask, road_mask, (unsigned)std::min(p.chunk_rows, n - q0), a,
                        ReadOut{readout, nullptr, read_at, q0, n}, BCRows{rows, count, q0, n});
}

}  // namespace

long long bc_blob_floats(int dim, int num_stack, int fusion_layers, int branch_layers, int head_layers, int n_components) {
    const int n_self = fusion_layers + 2 * branch_layers;
    return dim == 128 ? bc_layout<4>(num_stack, n_self, head_layers, n_components).total
                      : bc_layout<2>(num_stack, n_self, head_layers, n_components).total;
}

long long bc_scratch_floats(int dim, int max_agents, int chunk_rows) { return (long long)chunk_rows * 3 * (max_agents + ROADS) * dim; }

void launch_bc_forward(const gd_bc_policy &p, int dim, hipStream_t st, const float *obs, const unsigned char *partner_mask,
                       const unsigned char *road_mask, int n, bool deterministic, const float *u, const float *z,
                       const float *expert_actions, const gd_bc_outputs &out, const gd_bc_readout *readout,
                       const unsigned char *dead) {
    const BCHeadArgs a = head_args(p, deterministic, u, z, expert_actions, out);
    if (dim == 128)
        forward<4>(p, st, obs, partner_mask, road_mask, n, a, readout, dead);
    else
        forward<2>(p, st, obs, partner_mask, road_mask, n, a, readout, dead);
}

void launch_bc_forward_rows(const gd_bc_policy &p, int dim, hipStream_t st, const float *obs, const unsigned char *partner_mask,
                            const unsigned char *road_mask, int n, bool deterministic, const float *u, const float *z,
                            const float *expert_actions, const gd_bc_outputs &out, const int32_t *rows, const int32_t *count,
                            const gd_bc_readout *readout) {
    const BCHeadArgs a = head_args(p, deterministic, u, z, expert_actions, out);
    if (dim == 128)
        forward_rows<4>(p, st, obs, partner_mask, road_mask, n, a, rows, count, readout);
    else
        forward_rows<2>(p, st, obs, partner_mask, road_mask, n, a, rows, count, readout);
}

// ---- the forward's launches one by one at network_dim dim, for the backward's recomputation (and the probe's, at 64)

namespace {

template <int T>
void self_layer(const gd_bc_policy &p, hipStream_t st, const unsigned char *pm, const unsigned char *rm, int rows, int layer, float *X,
                float *Kb, float *Vb, float *osave, float *ml) {
    const Segs sg = bc_layer_segs<T>(p, layer);
    kv<T>(p, st, sg, (unsigned)rows, X, Kb, Vb);
    if (osave)
        attn<T>(p, st, sg, pm, rm, (unsigned)rows, X, Kb, Vb, osave, ml);
    else
        attn<T>(p, st, sg, pm, rm, (unsigned)rows, X, Kb, Vb);
}

template <int T>
void head_of_chunk(const gd_bc_policy &p, hipStream_t st, const unsigned char *partner_mask, const unsigned char *road_mask, int r0,
                   int rows, const BCHeadArgs &a, const float *X, const float *Kb, const float *Vb) {
    const int A = p.max_agents, R = p.num_stack;
    head<T>(p, st, partner_mask + (size_t)r0 * R * (A - 1), road_mask + (size_t)r0 * R * ROADS, (unsigned)rows,
            offset(a, r0, A, BCEnc<T>::CTX), X, Kb, Vb);
}

}  // namespace

void launch_bc_embed(const gd_bc_policy &p, int dim, hipStream_t st, const float *obs, int rows, float *X) {
    if (dim == 128)
        embed<4>(p, st, obs, (unsigned)rows, X);
    else
        embed<2>(p, st, obs, (unsigned)rows, X);
}

void launch_bc_self_layer(const gd_bc_policy &p, int dim, hipStream_t st, const unsigned char *pm, const unsigned char *rm, int rows,
                          int layer, float *X, float *Kb, float *Vb, float *osave, float *ml) {
    if (dim == 128)
        self_layer<4>(p, st, pm, rm, rows, layer, X, Kb, Vb, osave, ml);
    else
        self_layer<2>(p, st, pm, rm, rows, layer, X, Kb, Vb, osave, ml);
}

void launch_bc_cross_kv(const gd_bc_policy &p, int dim, hipStream_t st, int rows, const float *X, float *Kb, float *Vb) {
    if (dim == 128)
        kv<4>(p, st, bc_cross_segs<4>(p), (unsigned)rows, X, Kb, Vb);
    else
        kv<2>(p, st, bc_cross_segs<2>(p), (unsigned)rows, X, Kb, Vb);
}

// the masks, u, z, expert_actions and every output are the WHOLE call's; the chunk is its rows r0 .. r0 + rows
void launch_bc_head(const gd_bc_policy &p, int dim, hipStream_t st, const unsigned char *partner_mask, const unsigned char *road_mask,
                    int r0, int rows, bool deterministic, const float *u, const float *z, const float *expert_actions,
                    const gd_bc_outputs &out, const float *X, const float *Kb, const float *Vb) {
    const BCHeadArgs a = head_args(p, deterministic, u, z, expert_actions, out);
    if (dim == 128)
        head_of_chunk<4>(p, st, partner_mask, road_mask, r0, rows, a, X, Kb, Vb);
    else
        head_of_chunk<2>(p, st, partner_mask, road_mask, r0, rows, a, X, Kb, Vb);
}

void launch_bc_eval_accumulate(hipStream_t st, int n, const float *nll, const float *actions, const float *expert_actions,
                               float *acc) {
    hipLaunchKernelGGL(k_bc_eval_acc, dim3(1), dim3(64), 0, st, n, nll, actions, expert_actions, acc);
}

}  // namespace gd
