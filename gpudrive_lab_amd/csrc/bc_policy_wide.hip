// Device BC policy forward at network_dim = 128 (gd_bc_forward_dim, gd_bc_forward_rows_dim, gd_bc_rollout_dim): the model of
// the reference's sweep (baselines/il/sweep.yaml: network_dim 128, head_dim 64, num_layer [4, 3]).  bc_policy.hip's forward
// with every encoder width doubled; those kernels are left as they are and these stand beside them (bc_tile_wide.hpp).
// A token row is 128 floats; a wave holds 32 tokens transposed in four 16-register accumulators per lane.  Per chunk of
// gd_bc_policy.chunk_rows samples the launches are:
//   k_bcw_embed  a wave per 32 tokens of one kind: four Linear -> LayerNorm -> tanh.  Owns X[b][token].
//   k_bcw_kv     a wave per 32 tokens: K = Wk LN(x) + bk, V = Wv LN(x) + bv.  Owns K[b][token], V[b][token].
//   k_bcw_attn   a wave per 32 queries of one (sample, segment): q = (Wq LN(x) + bq) * 32^-1/2 (one multiplication by the
//                nearest float32), then per head the streamed softmax of k_bc_attn over the segment's keys in tiles of 32,
//                ascending.  A head has 32 channels and IS tile t = hd: S^T = K Q^T is 16 k-steps into one accumulator, and
//                O^T += V^T P^T fills all 32 rows of its accumulator (no half-empty product as at 64).  A masked key's score is
//                -FLT_MAX, keys past the segment's end do not exist.  Then o_proj + x, and the MLP + its input: ONE launch
//                holds the layer (x is read again for the residual instead of being kept across the heads).
//   k_bcw_head   a workgroup of 128 threads per sample, a thread per encoder feature: both cross attentions, the 384-wide
//                context, the 64-wide GMM head (threads 0 .. 63), bc_rule.hpp and every output of the row.
// 2 F + 2 S + 3 launches per chunk for F fusion and S branch layers, as at 64.  Every sum has one owner and a fixed order; no
// atomics; no host synchronisation; every byte of every output given is stored on every call.  The list instantiations
// (the pack of the last parameters is one BCRows) are the forward on a row list, by bc_policy.hip's rules.
#include "bc_tile_wide.hpp"

namespace gd {

namespace {

// grid (1 + ceil((A - 1) / 32) + 7, rows): tile 0 is the ego, then the partner tiles, then the road tiles
template <class... List>
__global__ __launch_bounds__(64) void k_bcw_embed(BCDims d, BCLayout L, const float *__restrict__ blob, const float *__restrict__ obs,
                                                  float *__restrict__ X, List... lr) {
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
    f16v a[TW], o[TW];
    if (kind == 2)
        embed_first128<ROAD_K>(x, d.D, d.R, EGO_K + PARTNER_K * (d.A - 1), ec, w0, rest, a, lane, h);
    else
        embed_first128<PARTNER_K>(x, d.D, d.R, kind == 0 ? 0 : EGO_K, ec, w0, rest, a, lane, h);
    layer_norm128(a, rest + FW, rest + 2 * FW, h);
#pragma unroll
    for (int t = 0; t < TW; t++)
#pragma unroll
        for (int r = 0; r < 16; r++) a[t][r] = tanhf(a[t][r]);
    for (int i = 0; i < 3; i++) {
        const float *__restrict__ w = rest + 3 * FW + i * (W128 + 3 * FW);
        linear128(a, w, w + W128, o, lane, h);
        layer_norm128(o, w + W128 + FW, w + W128 + 2 * FW, h);
#pragma unroll
        for (int t = 0; t < TW; t++)
#pragma unroll
            for (int r = 0; r < 16; r++) a[t][r] = tanhf(o[t][r]);
    }
    const int tok = (kind == 0 ? 0 : kind == 1 ? 1 : d.A) + e;
    if (live) store_tok128(X + ((size_t)slot * d.L + tok) * FW, a, h);
}

// grid (sum of tiles, rows).  Reads and writes the scratch only: b is the slot
template <class... List>
__global__ __launch_bounds__(64) void k_bcw_kv(BCDims d, Segs sg, const float *__restrict__ blob, const float *__restrict__ X,
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
    const size_t at = ((size_t)b * d.L + s.tok0 + (live ? j : s.ntok - 1)) * FW;
    f16v x[TW], o[TW];
    load_tok128(X + at, x, h);
    layer_norm128(x, blob + s.ng, blob + s.nb, h);
    linear128(x, blob + s.kw, blob + s.kb, o, lane, h);
    if (live) store_tok128(Kb + at, o, h);
    linear128(x, blob + s.vw, blob + s.vb, o, lane, h);
    if (live) store_tok128(Vb + at, o, h);
}

// grid (sum of tiles, rows).  List = (BCRows): the masks are the whole call's, X / K / V are indexed by slot
template <class... List>
__global__ __launch_bounds__(64) void k_bcw_attn(BCDims d, Segs sg, const float *__restrict__ blob,
                                                 const unsigned char *__restrict__ pm, const unsigned char *__restrict__ rm,
                                                 float *__restrict__ X, const float *__restrict__ Kb, const float *__restrict__ Vb,
                                                 List... lr) {
    __shared__ unsigned char msk[MAX_TOKENS];
    const int lane = threadIdx.x, h = lane >> 5, col = lane & 31;
    const int slot = blockIdx.y;
    const int b = bc_sample(slot, lr...);
    if constexpr (sizeof...(List) > 0) {
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
    const size_t seg_at = ((size_t)slot * d.L + s.tok0) * FW;
    float *xrow = X + seg_at + (size_t)(live ? qi : ntok - 1) * FW;
    f16v q[TW], o[TW];
    {
        f16v hn[TW];
        load_tok128(xrow, hn, h);
        layer_norm128(hn, w + WS_NG, w + WS_NB, h);
        linear128(hn, w + WS_QW, w + WS_QB, q, lane, h);
    }
#pragma unroll
    for (int t = 0; t < TW; t++)
#pragma unroll
        for (int r = 0; r < 16; r++) q[t][r] = q[t][r] * QSCALE_W;

#pragma unroll
    for (int hd = 0; hd < 4; hd++) {  // the head's 32 channels are tile hd: register r holds channel 32 hd + acc_row(r, h)
        float m = -INFINITY, l = 0.f;
        f16v O;
#pragma unroll
        for (int r = 0; r < 16; r++) O[r] = 0.f;
        for (int kb = 0; kb < ntok; kb += 32) {
            const int key = min(kb + col, ntok - 1);
            const float *__restrict__ kp = Kb + seg_at + (size_t)key * FW + 32 * hd + 4 * h;
            f4 kv[4];
#pragma unroll
            for (int g = 0; g < 4; g++) kv[g] = *reinterpret_cast<const f4 *>(kp + 8 * g);
            f16v sc;
#pragma unroll
            for (int r = 0; r < 16; r++) sc[r] = 0.f;
            // S^T[key][query]: k-step r contracts the channels 32 hd + acc_row(r, 0) and + 4
#pragma unroll
            for (int r = 0; r < 16; r++) sc = __builtin_amdgcn_mfma_f32_32x32x2f32(kv[r >> 2][r & 3], q[hd][r], sc, 0, 0, 0);
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
            // O^T[channel][query] += V^T P^T: P's registers are the B operand as they are; lane c supplies channel 32 hd + c
            const float *__restrict__ vp = Vb + seg_at + 32 * hd + col;
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int vk = min(kb + acc_row(r, h), ntok - 1);
                O = __builtin_amdgcn_mfma_f32_32x32x2f32(vp[(size_t)vk * FW], sc[r], O, 0, 0, 0);
            }
            m = mn;
        }
        const float lt = l + __shfl_xor(l, 32);
#pragma unroll
        for (int r = 0; r < 16; r++) o[hd][r] = O[r] / lt;
    }

    f16v y[TW], z[TW];
    linear128(o, w + WS_OW, w + WS_OB, y, lane, h);
    load_tok128(xrow, z, h);  // the layer's input again: nobody else writes these rows
#pragma unroll
    for (int t = 0; t < TW; t++)
#pragma unroll
        for (int r = 0; r < 16; r++) {
            y[t][r] = y[t][r] + z[t][r];
            z[t][r] = y[t][r];
        }
    layer_norm128(z, w + WS_MG, w + WS_MB, h);
    linear128(z, w + WS_W1, w + WS_B1, o, lane, h);
#pragma unroll
    for (int t = 0; t < TW; t++)
#pragma unroll
        for (int r = 0; r < 16; r++) o[t][r] = gelu_erf(o[t][r]);
    linear128(o, w + WS_W2, w + WS_B2, z, lane, h);
#pragma unroll
    for (int t = 0; t < TW; t++)
#pragma unroll
        for (int r = 0; r < 16; r++) y[t][r] = y[t][r] + z[t][r];
    if (live) store_tok128(xrow, y, h);
}

// grid (rows), 128 threads.  List = (BCRows): the masks and every pointer of `a` are the whole call's, X / K / V by slot
template <class... List>
__global__ __launch_bounds__(128) void k_bcw_head(BCDims d, BCLayout L, BCHeadArgs a, const float *__restrict__ blob,
                                                  const unsigned char *__restrict__ pm, const unsigned char *__restrict__ rm,
                                                  const float *__restrict__ X, const float *__restrict__ Kb,
                                                  const float *__restrict__ Vb, List... lr) {
    __shared__ float sc[4][ROADS];
    __shared__ float ctx[CTXW];
    __shared__ float vec[FW];
    __shared__ float raw[MAX_HEAD_OUT];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, slot = blockIdx.x, hd = tid >> 5;
    const int b = bc_sample(slot, lr...);
    if constexpr (sizeof...(List) > 0) {
        if (b < 0) return;
    }
    const size_t base = (size_t)slot * d.L * FW;
    const float xq = X[base + tid];  // ro_attn's token 0: the query of both cross attentions and the context's first third
    ctx[tid] = xq;
    for (int ci = 0; ci < 2; ci++) {
        const int tok0 = ci ? d.A : 1, nk = ci ? ROADS : d.A - 1;
        const float *__restrict__ w = blob + L.cross[ci];
        const float *__restrict__ wb = w + WC_BODY;  // the fields WS_* of a self layer follow the two norms
        const float qn = block_ln128(xq, w + WC_QG, w + WC_QB, tid, vec);
        const float qv = block_matvec128(wb + WS_QW, wb + WS_QB, qn, tid, vec) * QSCALE_W;
        vec[tid] = qv;
        __syncthreads();
        for (int j = tid; j < nk; j += 128) {
            const float *__restrict__ kp = Kb + base + (size_t)(tok0 + j) * FW;
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
        for (int j = 0; j < nk; j++) o = o + sc[hd][j] * Vb[base + (size_t)(tok0 + j) * FW + tid];
        const float y = block_matvec128(wb + WS_OW, wb + WS_OB, o, tid, vec) + xq;
        float zz = block_ln128(y, wb + WS_MG, wb + WS_MB, tid, vec);
        zz = gelu_erf(block_matvec128(wb + WS_W1, wb + WS_B1, zz, tid, vec));
        zz = block_matvec128(wb + WS_W2, wb + WS_B2, zz, tid, vec);
        ctx[FW * (1 + ci) + tid] = y + zz;
        __syncthreads();
    }
    // the GMM head, 64 wide: threads 0 .. 63 hold a feature each
    float hcur = 0.f;
    if (tid < F) {
        hcur = blob[L.head_in_b + tid];
        for (int k = 0; k < CTXW; k++) hcur = hcur + blob[L.head_in_w + k * F + tid] * ctx[k];
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
        for (int i = tid; i < CTXW; i += 128) a.context[(size_t)b * CTXW + i] = ctx[i];
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

// one chunk: the slots' samples are rows r0 .. (List empty; every pointer already advanced to r0) or the list's (List = BCRows)
template <class... List>
void launch_chunk(const gd_bc_policy &p, hipStream_t st, const float *obs, const unsigned char *pm, const unsigned char *rm,
                  unsigned slots, const BCHeadArgs &a, List... lr) {
    const BCDims d = bc_dims(p);
    const BCLayout L = bc_layout_wide(p);
    const size_t per = (size_t)p.chunk_rows * d.L * FW;
    float *X = p.scratch, *Kb = p.scratch + per, *Vb = p.scratch + 2 * per;
    const unsigned etiles = (unsigned)(1 + (d.A - 1 + 31) / 32 + (ROADS + 31) / 32);
    hipLaunchKernelGGL(k_bcw_embed<List...>, dim3(etiles, slots), dim3(64), 0, st, d, L, p.blob, obs, X, lr...);
    for (int i = 0; i < p.fusion_layers + p.branch_layers; i++) {
        const Segs sg = bc_layer_segs_wide(p, i);
        unsigned tiles = 0;
        for (int k = 0; k < sg.n; k++) tiles += (unsigned)sg.s[k].tiles;
        hipLaunchKernelGGL(k_bcw_kv<List...>, dim3(tiles, slots), dim3(64), 0, st, d, sg, p.blob, X, Kb, Vb, lr...);
        hipLaunchKernelGGL(k_bcw_attn<List...>, dim3(tiles, slots), dim3(64), 0, st, d, sg, p.blob, pm, rm, X, Kb, Vb, lr...);
    }
    const Segs cross = bc_cross_segs_wide(p);
    hipLaunchKernelGGL(k_bcw_kv<List...>, dim3((unsigned)(cross.s[0].tiles + cross.s[1].tiles), slots), dim3(64), 0, st, d, cross,
                       p.blob, X, Kb, Vb, lr...);
    hipLaunchKernelGGL(k_bcw_head<List...>, dim3(slots), dim3(128), 0, st, d, L, a, p.blob, pm, rm, X, Kb, Vb, lr...);
}

}  // namespace

long long bc_blob_floats_wide(int num_stack, int fusion_layers, int branch_layers, int head_layers, int n_components) {
    return bc_layout_wide(num_stack, fusion_layers + 2 * branch_layers, head_layers, n_components).total;
}

long long bc_scratch_floats_wide(int max_agents, int chunk_rows) { return (long long)chunk_rows * 3 * (max_agents + ROADS) * FW; }

void launch_bc_forward_wide(const gd_bc_policy &p, hipStream_t st, const float *obs, const unsigned char *partner_mask,
                            const unsigned char *road_mask, int n, bool deterministic, const float *u, const float *z,
                            const float *expert_actions, const gd_bc_outputs &out) {
    const BCDims d = bc_dims(p);
    const int A = p.max_agents, C = p.n_components;
    for (int r0 = 0; r0 < n; r0 += p.chunk_rows) {
        const int rows = std::min(p.chunk_rows, n - r0);
        gd_bc_outputs o{};
        o.context = out.context ? out.context + (size_t)r0 * CTXW : nullptr;
        o.means = out.means ? out.means + (size_t)r0 * 3 * C : nullptr;
        o.log_covariances = out.log_covariances ? out.log_covariances + (size_t)r0 * 3 * C : nullptr;
        o.covariances = out.covariances ? out.covariances + (size_t)r0 * 3 * C : nullptr;
        o.weights = out.weights ? out.weights + (size_t)r0 * C : nullptr;
        o.actions = out.actions ? out.actions + (size_t)r0 * 3 : nullptr;
        o.nll = out.nll ? out.nll + r0 : nullptr;
        o.ego_attn_score = out.ego_attn_score ? out.ego_attn_score + (size_t)r0 * 4 * (A - 1) : nullptr;
        o.component = out.component ? out.component + r0 : nullptr;
        const BCHeadArgs a = head_args(p, deterministic, u ? u + r0 : nullptr, z ? z + (size_t)r0 * 3 : nullptr,
                                       expert_actions ? expert_actions + (size_t)r0 * 3 : nullptr, o);
        launch_chunk(p, st, obs + (size_t)r0 * d.R * d.D, partner_mask + (size_t)r0 * d.R * (A - 1),
                     road_mask + (size_t)r0 * d.R * ROADS, (unsigned)rows, a);
    }
}

// every chunk of list positions with the full forward's grids: the host does not know the list's length
void launch_bc_forward_rows_wide(const gd_bc_policy &p, hipStream_t st, const float *obs, const unsigned char *partner_mask,
                                 const unsigned char *road_mask, int n, bool deterministic, const float *u, const float *z,
                                 const float *expert_actions, const gd_bc_outputs &out, const int32_t *rows, const int32_t *count) {
    const BCHeadArgs a = head_args(p, deterministic, u, z, expert_actions, out);
    for (int q0 = 0; q0 < n; q0 += p.chunk_rows) {
        const unsigned slots = (unsigned)std::min(p.chunk_rows, n - q0);
        launch_chunk(p, st, obs, partner_mask, road_mask, slots, a, BCRows{rows, count, q0, n});
    }
}

}  // namespace gd
