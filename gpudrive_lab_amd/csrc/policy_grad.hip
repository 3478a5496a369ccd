// Device policy backward (gd_policy_backward): the parameter gradients of the late-fusion actor-critic (policy.hip) from the
// features, logits and pool winners that gd_policy_evaluate saved, float32 throughout, as three launches:
//   k_pg_stats       a lane per row: (max, log-sum, entropy) of the row's logits (policy_grad_rule.hpp) and its upstream gradients
//                    and clamped action, to rowstat [N][8].
//   k_pg_accumulate  P workgroups of four waves; workgroup p takes the rows p, p + P, p + 2P, .. in ascending order and keeps
//                    its sums over them in registers (and, for the actor and critic weights, whose count follows n_actions, in
//                    its own slice of `partials`, each element read and written by one fixed lane).  Per row, through LDS:
//                      dlogits (the rule; d_value is row NA), hidden = Ws f + bs, dhidden = [Wa; Wc]^T dlogits,
//                      dfeatures = Ws^T dhidden;  dWs += dhidden x f, dWa += dlogits x hidden, the biases likewise;
//                    then the embedders.  The max-pool hands feature j's gradient to ONE entity, winners[j], so a wave (lane
//                    = first-layer feature) recomputes z = W1 x + b1, the LayerNorm and t = tanh(.) of that entity only, adds
//                    dpool_j t to row j of dW2 and pushes dpool_j W2[j][.] back through the tanh, the LayerNorm (biased
//                    variance, eps 1e-5) and the first layer.  Wave w owns the pooled features j = w, w + 4, ..  The ego
//                    embedder is the same with one entity and all 64 features at once.  Nothing of size N x entities x 64
//                    exists.  Workgroup p stores every element of partials[p] (zeros when it has no row).
//   k_pg_reduce      a lane per parameter: grad[e] = partials[0][e] + partials[1][e] + .. in that order.
// The weights are read in the state dict's natural layout (gd_policy_grad.params), which is also the layout of grad.
// No atomics: every sum has one owner and a fixed order, so equal inputs give equal bits.  Accumulations are fmaf; everything
// else rounds every operation (-ffp-contract=off).  Every byte of rowstat, partials and grad is stored on every call.
// Training-mode dropout (gd_policy_backward_dropout) is the DROP instantiation of k_pg_accumulate: the masks of
// the evaluate call whose index is in gd_dropout.used are recomputed (dropout_rule.hpp; a lane is a feature at all four sites,
// so one Philox call per lane and site) -- the recomputed hidden and tanh outputs are masked before they enter dWa, dWc and
// dW2, and the gradients that pass a mask (dhidden, the gradient at the tanh's output) are multiplied by mask * scale.
#include <hip/hip_runtime.h>

#include "dropout_rule.hpp"
#include "engine.hpp"
#include "policy_grad_rule.hpp"

namespace gd {

namespace {

namespace DR = dropout_rule;

// DROP: the mask of one row of one call
struct DropCall {
    DR::Args a;
    uint64_t call;
    uint32_t row;
};

constexpr int F = 64, HID = 128, FEAT = 192, ROADS = 200, MAX_ACTIONS = 1024;
constexpr int NT = 256, NW = 4, OWN = F / NW;  // lanes and waves of k_pg_accumulate; pooled features a wave owns
constexpr float LN_EPS = 1e-5f;

// offsets into params and grad, in floats: the state dict in policy.py's expected_shapes order, each tensor row-major
struct GradLayout {
    int k[3];                                       // first-layer width of ego, partner, road
    int w1[3], b1[3], g[3], be[3], w2[3], b2[3];
    int ws, bs, wa, ba, wc, bc, total;
};

// (constexpr: the kernels, instantiated per ego width, take every offset before the actor's bias as a constant)
constexpr GradLayout grad_layout(int ego_width, int n_actions) {
    GradLayout L{};
    int o = 0;
    L.k[0] = ego_width, L.k[1] = 6, L.k[2] = 13;
    for (int e = 0; e < 3; e++) {
        L.w1[e] = o, o += F * L.k[e];
        L.b1[e] = o, o += F;
        L.g[e] = o, o += F;
        L.be[e] = o, o += F;
        L.w2[e] = o, o += F * F;
        L.b2[e] = o, o += F;
    }
    L.ws = o, o += HID * FEAT;
    L.bs = o, o += HID;
    L.wa = o, o += n_actions * HID;
    L.ba = o, o += n_actions;
    L.wc = o, o += HID;
    L.bc = o, o += 1;
    L.total = o;
    return L;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) v = v + __shfl_xor(v, d);
    return v;
}

// rowstat [N][8]: m, logS, H, d_logprob, d_entropy, d_value, the clamped action (as float: below 2^24), 0
constexpr int RS = 8;

__global__ __launch_bounds__(64) void k_pg_stats(int n, int na, const float *__restrict__ logits, const int64_t *__restrict__ actions,
                                                 const float *__restrict__ d_logprob, const float *__restrict__ d_entropy,
                                                 const float *__restrict__ d_value, float *__restrict__ rowstat) {
    const int row = blockIdx.x * 64 + threadIdx.x;
    if (row >= n) return;
    const float *__restrict__ l = logits + (size_t)row * na;
    const policy_grad_rule::Stats s = policy_grad_rule::stats(na, [&](int k) { return l[k]; });
    const int64_t a = actions[row];
    float *__restrict__ o = rowstat + (size_t)row * RS;
    o[0] = s.m, o[1] = s.logS, o[2] = s.H, o[3] = d_logprob[row], o[4] = d_entropy[row], o[5] = d_value[row];
    o[6] = (float)(int)(a < 0 ? 0 : a >= na ? na - 1 : a), o[7] = 0.f;  // (out of range: clamped, for memory safety only)
}

// The sums one lane (first-layer feature f = lane) keeps for one embedder of first-layer width K
template <int K>
struct EmbedAcc {
    float w2[OWN], w1[K], b1, g, be;
};

// The first layer's weights of feature f = lane, read once per workgroup
template <int K>
struct EmbedW {
    float w1[K], b1, g, be;
};

template <int K>
__device__ __forceinline__ void load_embed(EmbedW<K> &w, EmbedAcc<K> &a, const float *__restrict__ prm, const GradLayout &L, int e,
                                           int lane) {
#pragma unroll
    for (int k = 0; k < K; k++) w.w1[k] = prm[L.w1[e] + lane * K + k], a.w1[k] = 0.f;
    w.b1 = prm[L.b1[e] + lane], w.g = prm[L.g[e] + lane], w.be = prm[L.be[e] + lane];
#pragma unroll
    for (int q = 0; q < OWN; q++) a.w2[q] = 0.f;
    a.b1 = a.g = a.be = 0.f;
}

// The recomputed forward of one entity row x[0..K): the normalised value and the tanh of feature f = lane, and 1 / std
template <int K>
__device__ __forceinline__ void entity_forward(const EmbedW<K> &w, const float (&x)[K], float &nrm, float &t, float &rstd) {
    float z = w.b1;
#pragma unroll
    for (int k = 0; k < K; k++) z = z + w.w1[k] * x[k];
    const float mean = wave_sum(z) * (1.f / 64.f);
    const float d = z - mean;
    rstd = 1.f / sqrtf(wave_sum(d * d) * (1.f / 64.f) + LN_EPS);
    nrm = d * rstd;
    t = tanhf(nrm * w.g + w.be);
}

// dt (the gradient at the tanh's output, feature f = lane) back through the tanh, the LayerNorm and the first layer
template <int K>
__device__ __forceinline__ void entity_backward(const EmbedW<K> &w, EmbedAcc<K> &a, const float (&x)[K], float nrm, float t,
                                                float rstd, float dt) {
    const float du = dt * (1.f - t * t);
    a.g = fmaf(du, nrm, a.g);
    a.be = a.be + du;
    const float dn = du * w.g;
    const float m1 = wave_sum(dn) * (1.f / 64.f);
    const float m2 = wave_sum(dn * nrm) * (1.f / 64.f);
    const float dz = rstd * ((dn - m1) - nrm * m2);
    a.b1 = a.b1 + dz;
#pragma unroll
    for (int k = 0; k < K; k++) a.w1[k] = fmaf(dz, x[k], a.w1[k]);
}

// One set embedder of one row: the OWN pooled features of wave wv, each at its winner
template <int K, bool DROP>
__device__ __forceinline__ void set_backward(const EmbedW<K> &w, EmbedAcc<K> &a, const float *__restrict__ rows, int count,
                                             const unsigned char *__restrict__ win, const float *__restrict__ dpool,
                                             const float *__restrict__ w2, int wv, int lane, const DropCall &dc, uint32_t site) {
    // lane l holds winners[l]; the next entity's row and W2 element are loaded while this one is worked on (at 1 wave per SIMD
    // nothing else hides the latency)
    const int mine = win[lane];
    auto entity = [&](int q) {
        const int e = __shfl(mine, wv + NW * q);
        return rows + (size_t)(e < count ? e : count - 1) * K;  // (memory safety: gd_policy_evaluate's winners are below count)
    };
    float xn[K];
    const float *__restrict__ xr = entity(0);
#pragma unroll
    for (int k = 0; k < K; k++) xn[k] = xr[k];
    float w2n = w2[wv * F + lane];
#pragma unroll 4
    for (int q = 0; q < OWN; q++) {
        const int j = wv + NW * q;
        float x[K];
#pragma unroll
        for (int k = 0; k < K; k++) x[k] = xn[k];
        const float w2j = w2n;
        const int qn = q + 1 < OWN ? q + 1 : q;  // (the last iteration loads its own again)
        xr = entity(qn);
#pragma unroll
        for (int k = 0; k < K; k++) xn[k] = xr[k];
        w2n = w2[(wv + NW * qn) * F + lane];
        float nrm, t, rstd;
        entity_forward<K>(w, x, nrm, t, rstd);
        const float dp = dpool[j];
        float tm = t, dt = dp * w2j;
        if constexpr (DROP) {
            // the winner's mask, feature f = lane (the index clamped as `entity` clamps it)
            const int e = __shfl(mine, j);
            const bool keep = DR::kept(dc.a.seed, dc.call, dc.row, site, (uint32_t)(e < count ? e : count - 1), lane, dc.a.threshold);
            tm = DR::apply(t, keep, dc.a.scale), dt = DR::apply(dt, keep, dc.a.scale);
        }
        // (a.w2 is indexed by the loop counter: select instead of a dynamic register index)
#pragma unroll
        for (int qq = 0; qq < OWN; qq++) a.w2[qq] = qq == q ? fmaf(dp, tm, a.w2[qq]) : a.w2[qq];
        entity_backward<K>(w, a, x, nrm, t, rstd, dt);
    }
}

// Four waves' sums of one per-feature quantity, added in wave order and stored by wave 0
__device__ __forceinline__ void store_wave_sum(float (*red)[F], float v, float *__restrict__ dst, int stride, int wv, int lane) {
    red[wv][lane] = v;
    __syncthreads();
    if (wv == 0) dst[lane * stride] = ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
    __syncthreads();
}

template <int K>
__device__ __forceinline__ void store_set(float (*red)[F], const EmbedAcc<K> &a, float *__restrict__ part, const GradLayout &L,
                                          int e, int wv, int lane) {
#pragma unroll
    for (int q = 0; q < OWN; q++) part[L.w2[e] + (wv + NW * q) * F + lane] = a.w2[q];
#pragma unroll
    for (int k = 0; k < K; k++) store_wave_sum(red, a.w1[k], part + L.w1[e] + k, K, wv, lane);
    store_wave_sum(red, a.b1, part + L.b1[e], 1, wv, lane);
    store_wave_sum(red, a.g, part + L.g[e], 1, wv, lane);
    store_wave_sum(red, a.be, part + L.be[e], 1, wv, lane);
}

// DROP: da and usedp are the rule's values and the device word that holds the evaluate call's index; without DROP they are
// not read
template <int EW, bool DROP>
__global__ __launch_bounds__(NT) void k_pg_accumulate(int n, int partners, int na, const float *__restrict__ prm,
                                                      const float *__restrict__ obs, const float *__restrict__ features, const float *__restrict__ logits,
                                                      const unsigned char *__restrict__ winners,
                                                      const float *__restrict__ rowstat, float *__restrict__ partials, DR::Args da,
                                                      const uint64_t *__restrict__ usedp) {
    __shared__ float s_f[FEAT], s_df[FEAT], s_hid[HID], s_dh[HID], s_dl[MAX_ACTIONS + 8];
    __shared__ float s_red[NW][F];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int P = gridDim.x;
    GradLayout L = grad_layout(EW, 0);  // folds to constants up to wa
    L.ba = L.wa + na * HID, L.wc = L.ba + na, L.bc = L.wc + HID, L.total = L.bc + 1;
    float *__restrict__ part = partials + (size_t)blockIdx.x * L.total;
    const size_t width = (size_t)EW + (size_t)6 * partners + (size_t)13 * ROADS;
    auto head_b = [&](int k) { return k < na ? L.ba + k : L.bc; };

    // the head's weight sums live in this workgroup's slice of partials; element (k, i) of [Wa; Wc] belongs to lane
    // 128 (k & 1) + i throughout
#pragma unroll 1
    for (int k = tid >> 7; k <= na; k += 2) part[(k < na ? L.wa + k * HID : L.wc) + (tid & (HID - 1))] = 0.f;
#pragma unroll 1
    for (int k = tid; k <= na; k += NT) part[head_b(k)] = 0.f;

    float a_ws[HID / NW][FEAT / F];  // dWs[wv + 4 i][lane + 64 j]
#pragma unroll
    for (int i = 0; i < HID / NW; i++)
#pragma unroll
        for (int j = 0; j < FEAT / F; j++) a_ws[i][j] = 0.f;
    float a_bs = 0.f, a_b2 = 0.f;  // dbs[tid] (tid < 128); db2 of embedder wv, feature lane (tid < 192)
    EmbedW<EW> w_ego;
    EmbedW<6> w_par;
    EmbedW<13> w_road;
    EmbedAcc<EW> a_ego;
    EmbedAcc<6> a_par;
    EmbedAcc<13> a_road;
    load_embed<EW>(w_ego, a_ego, prm, L, 0, lane);
    load_embed<6>(w_par, a_par, prm, L, 1, lane);
    load_embed<13>(w_road, a_road, prm, L, 2, lane);
    DropCall dc{da, 0, 0};
    if constexpr (DROP) dc.call = *usedp;

    for (int row = blockIdx.x; row < n; row += P) {
        // DROP: lanes i and 128 + i both hold the mask of hidden feature i
        bool keep_h = true;
        if constexpr (DROP) {
            dc.row = (uint32_t)row;
            keep_h = DR::kept(dc.a.seed, dc.call, dc.row, DR::SITE_SHARED, 0, tid & (HID - 1), dc.a.threshold);
        }
        // the row's features and dlogits
        if (tid < FEAT) s_f[tid] = features[(size_t)row * FEAT + tid];
        {
            const float *__restrict__ rs = rowstat + (size_t)row * RS;
            policy_grad_rule::Stats st;
            st.m = rs[0], st.logS = rs[1], st.H = rs[2];
            const float dlp = rs[3], dent = rs[4];
            const int a = (int)rs[6];
#pragma unroll 1
            for (int k = tid; k < na; k += NT) s_dl[k] = policy_grad_rule::dlogit(logits[(size_t)row * na + k], k == a, st, dlp, dent);
            if (tid < 8) s_dl[na + tid] = tid == 0 ? rs[5] : 0.f;
        }
        __syncthreads();
        // hidden (lanes 0..127) and dhidden (lanes 128..255)
        if (tid < HID) {
            const float *__restrict__ wr = prm + L.ws + tid * FEAT;
            float h = prm[L.bs + tid];
#pragma unroll 16
            for (int j = 0; j < FEAT; j++) h = fmaf(wr[j], s_f[j], h);
            if constexpr (DROP) h = DR::apply(h, keep_h, dc.a.scale);
            s_hid[tid] = h;
        } else {
            // [Wa; Wc] as NA + 1 rows, eight at a time with no remainder loop: past the end the row index stays at the critic's
            // and s_dl holds zeros, and fmaf(w, 0, d) is d
            const int i = tid - HID;
            float d = 0.f;
#pragma unroll 1
            for (int k0 = 0; k0 <= na; k0 += 8) {
#pragma unroll
                for (int u = 0; u < 8; u++) {
                    const int k = k0 + u;
                    d = fmaf(prm[(k < na ? L.wa + k * HID : L.wc) + i], s_dl[k], d);
                }
            }
            if constexpr (DROP) d = DR::apply(d, keep_h, dc.a.scale);
            s_dh[i] = d;
        }
        __syncthreads();
        // dfeatures, and the head's sums
        if (tid < FEAT) {
            float d = 0.f;
#pragma unroll 16
            for (int i = 0; i < HID; i++) d = fmaf(prm[L.ws + i * FEAT + tid], s_dh[i], d);
            s_df[tid] = d;
            a_b2 = a_b2 + d;
        }
        if (tid < HID) a_bs = a_bs + s_dh[tid];
        {
            float f[FEAT / F];
#pragma unroll
            for (int j = 0; j < FEAT / F; j++) f[j] = s_f[lane + F * j];
#pragma unroll
            for (int i = 0; i < HID / NW; i++) {
                const float d = s_dh[wv + NW * i];
#pragma unroll
                for (int j = 0; j < FEAT / F; j++) a_ws[i][j] = fmaf(d, f[j], a_ws[i][j]);
            }
        }
        {
            // element (k, i) of [Wa; Wc] belongs to lane 128 (k & 1) + i; four loads in flight, no remainder loop: past the
            // end the address stays at the critic's row and nothing is stored
            const int half = tid >> 7, i = tid & (HID - 1);
            const float hi = s_hid[i];
#pragma unroll 1
            for (int k0 = 0; k0 <= na; k0 += 8) {
                float v[4];
                int at[4];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int k = k0 + 2 * u + half;
                    at[u] = (k < na ? L.wa + k * HID : L.wc) + i;
                    v[u] = part[at[u]];
                }
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int k = k0 + 2 * u + half;
                    if (k <= na) part[at[u]] = fmaf(s_dl[k], hi, v[u]);
                }
            }
        }
#pragma unroll 1
        for (int k = tid; k <= na; k += NT) {
            const int at = head_b(k);
            part[at] = part[at] + s_dl[k];
        }
        __syncthreads();
        // the embedders: every wave recomputes the ego row (all 64 pooled features share it) and keeps its own rows of dW2;
        // wave 0 alone keeps the ego's first-layer sums
        const float *__restrict__ x = obs + (size_t)row * width;
        {
            float xe[EW];
#pragma unroll
            for (int k = 0; k < EW; k++) xe[k] = x[k];
            float nrm, t, rstd;
            entity_forward<EW>(w_ego, xe, nrm, t, rstd);
            float dt = 0.f;
#pragma unroll 16
            for (int j = 0; j < F; j++) dt = fmaf(s_df[j], prm[L.w2[0] + j * F + lane], dt);
            float tm = t;
            if constexpr (DROP) {
                const bool keep = DR::kept(dc.a.seed, dc.call, dc.row, DR::SITE_EGO, 0, lane, dc.a.threshold);
                tm = DR::apply(t, keep, dc.a.scale), dt = DR::apply(dt, keep, dc.a.scale);
            }
#pragma unroll
            for (int q = 0; q < OWN; q++) a_ego.w2[q] = fmaf(s_df[wv + NW * q], tm, a_ego.w2[q]);
            if (wv == 0) entity_backward<EW>(w_ego, a_ego, xe, nrm, t, rstd, dt);
        }
        const unsigned char *__restrict__ win = winners + (size_t)row * (2 * F);
        set_backward<6, DROP>(w_par, a_par, x + EW, partners, win, s_df + F, prm + L.w2[1], wv, lane, dc, DR::SITE_PARTNER);
        set_backward<13, DROP>(w_road, a_road, x + EW + 6 * partners, ROADS, win + F, s_df + 2 * F, prm + L.w2[2], wv, lane, dc,
                               DR::SITE_ROAD);
        // (the next row's first stage writes s_f and s_dl only, which nothing above reads after the last barrier)
    }

#pragma unroll
    for (int i = 0; i < HID / NW; i++)
#pragma unroll
        for (int j = 0; j < FEAT / F; j++) part[L.ws + (wv + NW * i) * FEAT + lane + F * j] = a_ws[i][j];
    if (tid < HID) part[L.bs + tid] = a_bs;
    if (tid < FEAT) part[(wv == 0 ? L.b2[0] : wv == 1 ? L.b2[1] : L.b2[2]) + lane] = a_b2;
    // ego: the rows of dW2 by their owners, the rest by wave 0
#pragma unroll
    for (int q = 0; q < OWN; q++) part[L.w2[0] + (wv + NW * q) * F + lane] = a_ego.w2[q];
    if (wv == 0) {
#pragma unroll
        for (int k = 0; k < EW; k++) part[L.w1[0] + lane * EW + k] = a_ego.w1[k];
        part[L.b1[0] + lane] = a_ego.b1, part[L.g[0] + lane] = a_ego.g, part[L.be[0] + lane] = a_ego.be;
    }
    store_set<6>(s_red, a_par, part, L, 1, wv, lane);
    store_set<13>(s_red, a_road, part, L, 2, wv, lane);
}

__global__ __launch_bounds__(256) void k_pg_reduce(int total, int P, const float *__restrict__ partials, float *__restrict__ grad) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    float s = partials[e];
    for (int p = 1; p < P; p++) s = s + partials[(size_t)p * total + e];
    grad[e] = s;
}

}  // namespace

long long policy_grad_floats(int ego_width, int n_actions) { return grad_layout(ego_width, n_actions).total; }

void launch_policy_backward(const gd_policy &p, const gd_policy_grad &g, hipStream_t st, const float *obs, const int64_t *actions,
                            const float *d_logprob, const float *d_entropy, const float *d_value, float *grad) {
    const GradLayout L = grad_layout(p.ego_width, p.n_actions);
    const int n = p.num_rows, na = p.n_actions, P = g.num_partials;
    hipLaunchKernelGGL(k_pg_stats, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, n, na, g.logits, actions, d_logprob, d_entropy,
                       d_value, g.rowstat);
    if (p.ego_width == 6)
        hipLaunchKernelGGL((k_pg_accumulate<6, false>), dim3((unsigned)P), dim3(NT), 0, st, n, p.max_agents - 1, na, g.params, obs,
                           g.features, g.logits, g.winners, g.rowstat, g.partials, DR::Args{}, (const uint64_t *)nullptr);
    else
        hipLaunchKernelGGL((k_pg_accumulate<9, false>), dim3((unsigned)P), dim3(NT), 0, st, n, p.max_agents - 1, na, g.params, obs,
                           g.features, g.logits, g.winners, g.rowstat, g.partials, DR::Args{}, (const uint64_t *)nullptr);
    hipLaunchKernelGGL(k_pg_reduce, dim3((unsigned)((L.total + 255) / 256)), dim3(256), 0, st, L.total, P, g.partials, grad);
}

// The masked backward: the masks of the evaluate call whose index is *d.used
void launch_policy_backward(const gd_policy &p, const gd_policy_grad &g, const gd_dropout &d, hipStream_t st, const float *obs,
                            const int64_t *actions, const float *d_logprob, const float *d_entropy, const float *d_value,
                            float *grad) {
    const GradLayout L = grad_layout(p.ego_width, p.n_actions);
    const int n = p.num_rows, na = p.n_actions, P = g.num_partials;
    const DR::Args da{d.seed, d.threshold, d.scale};
    hipLaunchKernelGGL(k_pg_stats, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, n, na, g.logits, actions, d_logprob, d_entropy,
                       d_value, g.rowstat);
    if (p.ego_width == 6)
        hipLaunchKernelGGL((k_pg_accumulate<6, true>), dim3((unsigned)P), dim3(NT), 0, st, n, p.max_agents - 1, na, g.params, obs,
                           g.features, g.logits, g.winners, g.rowstat, g.partials, da, (const uint64_t *)d.used);
    else
        hipLaunchKernelGGL((k_pg_accumulate<9, true>), dim3((unsigned)P), dim3(NT), 0, st, n, p.max_agents - 1, na, g.params, obs,
                           g.features, g.logits, g.winners, g.rowstat, g.partials, da, (const uint64_t *)d.used);
    hipLaunchKernelGGL(k_pg_reduce, dim3((unsigned)((L.total + 255) / 256)), dim3(256), 0, st, L.total, P, g.partials, grad);
}

}  // namespace gd
