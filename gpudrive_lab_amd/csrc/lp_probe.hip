// Device linear probe (gd_bc_hidden, gd_lp_forward, gd_lp_update, gd_lp_eval_accumulate): the reference's linear-probing loop
// (baselines/il/linear_probing.py:169-342, LinearProbPosition of gpudrive/integrations/il/linear_probing/lp_model.py) on the
// hidden states of the device BC policy.  The rule -- every rounding, the order of every sum -- is csrc/lp_rule.hpp.
//   the tap       per chunk of gd_bc_policy.chunk_rows samples bc_policy.hip's own launches run and STOP at the tapped block:
//                 launch_bc_embed and the fusion layers for fusion_attn (no branch layer, no cross attention, no head), the
//                 branch layers as well for ro_attn.  The block's last_hidden_state is then the first A tokens of X.
//   k_lp_copy     gd_bc_hidden only: those A tokens of every sample of the chunk to out [n][A][64], 16 bytes per lane.
//   k_lp_rows     grid (num_partials), one wave each.  Workgroup w takes the tiles w, w + num_partials, .. of the chunk in
//                 ascending order.  A tile is 32 rows: for 'other' the partner columns 32 i .. 32 i + 31 of one sample, which are
//                 the tokens 1 + column (one off the 32-token tiles the attention kernel wrote, and the last tile holds 31 rows:
//                 A - 1 is 63 or 127), for 'ego' token 0 of 32 consecutive samples.  Logits by bc_tile.hpp's linear from the
//                 probe's packed weights; the tile of logits goes through LDS so that a lane owns a whole row for the row rule;
//                 g and x (zeros for a row that is not selected) go through LDS again as the operands of the gradient's MFMA
//                 chain over the rows, whose accumulators start from the workgroup's partial and return to it after its last
//                 tile.  Lane c counts class c.  No atomics: a partial has one owner.
//                 The baseline probe (no backbone) is the same kernel with the tile gathered from obs instead of X.
//   k_lp_reduce   the partials in ascending order, M, the scaled gradient, the statistics; workgroup 0 also advances the step
//                 and the betas' running products (M > 0) or `skipped` (M == 0), or adds the batch to the evaluation's sums.
//   k_lp_adamw    a lane per parameter, predicated on the flag k_lp_reduce left: the weight to the flat layout and to its place
//                 in the packed form (computed, not looked up; a padding column of the packed form is never written).
// Every launch is on the caller's stream; no host synchronisation, no allocation; equal inputs, chunk_rows and num_partials
// give equal bits.
#include "bc_tile.hpp"
#include "lp_rule.hpp"

namespace gd {

namespace {

namespace R = lp_rule;
namespace P = ppo_rule;
constexpr int LDW = F + 1;  // a [32 rows][64] tile in LDS, padded against bank conflicts
constexpr int NT = 256;

struct LPArgs {
    int exp, model, K, A, Rs, D, L;  // K: in_features; Rs: num_stack; D: floats per obs row; L: tokens per sample in X
    int r0, rows;                    // the chunk: its first sample in the call and its samples
    int stats, want_grad;            // labels are given; the gradient's sums are wanted
    const float *packed, *X, *obs;   // obs: the CHUNK's (baseline only)
    const unsigned char *mask;       // the WHOLE call's, as labels and the three row outputs
    const int64_t *labels;
    float *logits, *loss_row;
    int64_t *pred;
    float *part_f;
    double *part_d;
    int *part_i;
};

__device__ __forceinline__ int packed_at(int o, int i) {
    const int t2 = o >> 5, c = o & 31, t = i >> 5, w = i & 31;
    const int h = (w >> 2) & 1, r = (w & 3) + 4 * (w >> 3);
    return ((t2 * 2 + t) * 16 + r) * 64 + c + 32 * h;
}

__global__ __launch_bounds__(256) void k_lp_zero(float *__restrict__ pf, long long nf, double *__restrict__ pd, long long nd,
                                                 int *__restrict__ pi, long long ni) {
    const long long i0 = (long long)blockIdx.x * 256 + threadIdx.x, stride = (long long)gridDim.x * 256;
    for (long long i = i0; i < nf; i += stride) pf[i] = 0.f;
    for (long long i = i0; i < nd; i += stride) pd[i] = 0.0;
    for (long long i = i0; i < ni; i += stride) pi[i] = 0;
}

// grid (ceil(A * 16 / 256), rows): 16 lanes per token
__global__ __launch_bounds__(256) void k_lp_copy(int A, int L, int r0, const float *__restrict__ X, float *__restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (i >= A * 16) return;
    const f4 v = *reinterpret_cast<const f4 *>(X + (size_t)b * L * F + (size_t)i * 4);
    *reinterpret_cast<f4 *>(out + (size_t)(r0 + b) * A * F + (size_t)i * 4) = v;
}

// BASE: the baseline probe's gather from obs instead of the tapped tokens
template <bool BASE>
__global__ __launch_bounds__(64) void k_lp_rows(LPArgs a) {
    __shared__ float ldZ[32 * LDW], ldG[32 * LDW], ldX[32 * LDW];
    __shared__ float s_loss[32];
    __shared__ int s_pred[32], s_lab[32], s_bad[32];
    const int lane = threadIdx.x, h = lane >> 5, col = lane & 31;
    const bool other = a.exp == R::EXP_OTHER;
    const int per = other ? a.A - 1 : 1;            // rows per sample
    const int tps = other ? (a.A - 1 + 31) / 32 : 0;  // tiles per sample ('other')
    const int total = other ? a.rows * tps : (a.rows + 31) / 32;
    const int GF = F * a.K + F;
    float *__restrict__ pf = a.part_f ? a.part_f + (size_t)blockIdx.x * GF : nullptr;
    const int ktiles = (a.K + 31) / 32;

    // the gradient's accumulators: [t2][tk] tiles of dW, and db of output `lane`
    f16v acc[2][2];
    float db = 0.f;
    double loss = 0.0, ood_loss = 0.0;
    int n_correct = 0, n_rows = 0, n_bad = 0, n_ood_correct = 0, n_ood_rows = 0;
    int cnt[R::N_COUNTERS];
#pragma unroll
    for (int k = 0; k < R::N_COUNTERS; k++) cnt[k] = 0;
    if (a.want_grad) {
#pragma unroll
        for (int t2 = 0; t2 < 2; t2++)
#pragma unroll
            for (int tk = 0; tk < 2; tk++) {
                const int i = 32 * tk + col;
#pragma unroll
                for (int r = 0; r < 16; r++) acc[t2][tk][r] = i < a.K ? pf[(32 * t2 + acc_row(r, h)) * a.K + i] : 0.f;
            }
        db = pf[F * a.K + lane];
    }

    for (int id = blockIdx.x; id < total; id += gridDim.x) {
        // this lane's row: sample b of the chunk, row j of the sample
        int b, j;
        bool live;
        if (other) {
            b = id / tps, j = (id % tps) * 32 + col;
            live = j < per;
            if (!live) j = per - 1;  // a lane past the end computes the last row again and stores nothing
        } else {
            b = id * 32 + col, j = 0;
            live = b < a.rows;
            if (!live) b = a.rows - 1;
        }
        const size_t gr = (size_t)(a.r0 + b) * per + j;  // the row in the whole call
        f16v x[2], z[2];
        if constexpr (BASE) {
            const float *__restrict__ o = a.obs + (size_t)b * a.Rs * a.D;
#pragma unroll
            for (int t = 0; t < 2; t++)
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const int k = 32 * t + acc_row(r, h);
                    float v = 0.f;
                    if (k < a.K) {
                        if (other) {  // [ego 6 | partner j's 6] per time index
                            const int tm = k / 12, c = k % 12;
                            v = o[(size_t)tm * a.D + (c < 6 ? c : EGO_K + PARTNER_K * j + (c - 6))];
                        } else {
                            v = o[(size_t)(k / 6) * a.D + k % 6];
                        }
                    }
                    x[t][r] = v;
                }
        } else {
            load_tok(a.X + ((size_t)b * a.L + (other ? 1 + j : 0)) * F, x, h);
        }
        linear(x, a.packed, a.packed + W64, z, lane, h);
        if (a.logits && live) store_tok(a.logits + gr * F, z, h);

        __syncthreads();  // the tile before this one has been read
#pragma unroll
        for (int t = 0; t < 2; t++)
#pragma unroll
            for (int r = 0; r < 16; r++) ldZ[col * LDW + 32 * t + acc_row(r, h)] = z[t][r];
        __syncthreads();
        const float *__restrict__ zr = ldZ + col * LDW;
        const R::Row row = R::row([&](int c) { return zr[c]; });  // both lanes of the row compute the same values
        if (a.pred && live && h == 0) a.pred[gr] = row.pred;
        if (!a.stats) continue;

        const long long label = a.labels[gr];
        const bool ok = R::label_ok(label);
        const bool sel = live && R::selected(a.exp, a.mask[gr]);
        const bool use = sel && ok;
        const int lab = ok ? (int)label : 0;
        const float lr = ok ? R::loss_row(row, zr[lab]) : 0.f;
        if (a.loss_row && live && h == 0) a.loss_row[gr] = lr;
#pragma unroll 1
        for (int c = 32 * h; c < 32 * h + 32; c++) ldG[col * LDW + c] = use ? R::grad(row, zr[c], c == lab) : 0.f;
#pragma unroll
        for (int t = 0; t < 2; t++)
#pragma unroll
            for (int r = 0; r < 16; r++) ldX[col * LDW + 32 * t + acc_row(r, h)] = use ? x[t][r] : 0.f;
        if (h == 0) s_loss[col] = lr, s_pred[col] = row.pred, s_lab[col] = use ? lab : -1, s_bad[col] = sel && !ok;
        __syncthreads();

        if (a.want_grad) {
            // dW[o][i] += sum over the tile's rows, ascending, of g[row][o] x[row][i]
#pragma unroll
            for (int t2 = 0; t2 < 2; t2++)
#pragma unroll
                for (int tk = 0; tk < 2; tk++) {
                    if (tk >= ktiles) continue;
#pragma unroll
                    for (int s = 0; s < 16; s++)
                        acc[t2][tk] = __builtin_amdgcn_mfma_f32_32x32x2f32(ldG[(2 * s + h) * LDW + 32 * t2 + col],
                                                                           ldX[(2 * s + h) * LDW + 32 * tk + col], acc[t2][tk], 0, 0, 0);
                }
            for (int rr = 0; rr < 32; rr++) db = db + ldG[rr * LDW + lane];
        }
        // lane c counts class c; the scalar sums are the same in every lane
        for (int rr = 0; rr < 32; rr++) {
            n_bad += s_bad[rr];
            const int l = s_lab[rr];
            if (l < 0) continue;
            const int p = s_pred[rr];
            const bool od = R::ood(a.exp, l);
            loss += (double)s_loss[rr];
            n_rows++, n_correct += p == l;
            cnt[R::C_TP] += p == lane && l == lane, cnt[R::C_PRED] += p == lane, cnt[R::C_LABEL] += l == lane;
            if (od) {
                ood_loss += (double)s_loss[rr];
                n_ood_rows++, n_ood_correct += p == l;
                cnt[R::C_OOD_TP] += p == lane && l == lane, cnt[R::C_OOD_PRED] += p == lane, cnt[R::C_OOD_LABEL] += l == lane;
            }
        }
    }

    if (!a.stats) return;
    if (a.want_grad) {
#pragma unroll
        for (int t2 = 0; t2 < 2; t2++)
#pragma unroll
            for (int tk = 0; tk < 2; tk++) {
                const int i = 32 * tk + col;
                if (i < a.K) {
#pragma unroll
                    for (int r = 0; r < 16; r++) pf[(32 * t2 + acc_row(r, h)) * a.K + i] = acc[t2][tk][r];
                }
            }
        pf[F * a.K + lane] = db;
    }
    int *__restrict__ pi = a.part_i + (size_t)blockIdx.x * R::PART_INTS;
#pragma unroll
    for (int k = 0; k < R::N_COUNTERS; k++) pi[R::N_HEAD + k * R::CLASSES + lane] += cnt[k];
    if (lane == 0) {
        double *__restrict__ pd = a.part_d + (size_t)blockIdx.x * R::PART_DOUBLES;
        pd[0] += loss, pd[1] += ood_loss;
        pi[R::N_CORRECT] += n_correct, pi[R::N_ROWS] += n_rows, pi[R::N_BAD] += n_bad;
        pi[R::N_OOD_CORRECT] += n_ood_correct, pi[R::N_OOD_ROWS] += n_ood_rows;
    }
}

struct LPReduce {
    int P, K, train;  // train: advance the optimiser's scalars (workgroup 0); otherwise add the batch to acc
    double beta1, beta2;
    const float *part_f;
    const double *part_d;
    const int *part_i;
    float *grad, *stats, *scal;
    double *sums, *beta_pow;
    int *counts, *step;
    int *acc;  // the evaluation's accumulators
};

// grid (ceil((64 K + 64) / 256)) with the gradient, (1) without
__global__ __launch_bounds__(NT) void k_lp_reduce(LPReduce a) {
    __shared__ int s_cnt[R::N_COUNTERS][R::CLASSES];
    __shared__ int s_m;
    const int tid = threadIdx.x;
    if (tid == 0) {
        int m = 0;
        for (int w = 0; w < a.P; w++) m += a.part_i[(size_t)w * R::PART_INTS + R::N_ROWS];
        s_m = m;
    }
    __syncthreads();
    const int M = s_m;
    const int GF = F * a.K + F;
    if (a.grad && M > 0) {
        const int e = blockIdx.x * NT + tid;
        if (e < GF) {
            float s = a.part_f[e];
            for (int w = 1; w < a.P; w++) s = s + a.part_f[(size_t)w * GF + e];
            a.grad[e] = R::scaled(s, M);
        }
    }
    if (blockIdx.x != 0) return;
    for (int i = tid; i < R::N_COUNTERS * R::CLASSES; i += NT) {
        int s = 0;
        for (int w = 0; w < a.P; w++) s += a.part_i[(size_t)w * R::PART_INTS + R::N_HEAD + i];
        s_cnt[i / R::CLASSES][i % R::CLASSES] = s;
    }
    __syncthreads();
    if (tid != 0) return;
    double loss = 0.0, ood_loss = 0.0;
    int correct = 0, bad = 0, ood_correct = 0, ood_rows = 0;
    for (int w = 0; w < a.P; w++) {
        const int *__restrict__ pi = a.part_i + (size_t)w * R::PART_INTS;
        loss += a.part_d[(size_t)w * R::PART_DOUBLES], ood_loss += a.part_d[(size_t)w * R::PART_DOUBLES + 1];
        correct += pi[R::N_CORRECT], bad += pi[R::N_BAD], ood_correct += pi[R::N_OOD_CORRECT], ood_rows += pi[R::N_OOD_ROWS];
    }
    float st[3] = {0.f, 0.f, 0.f};
    if (M > 0) {
        st[0] = R::loss_of(loss, M), st[1] = R::accuracy_of(correct, M);
        st[2] = R::macro_f1([&](int c) { return s_cnt[R::C_TP][c]; }, [&](int c) { return s_cnt[R::C_PRED][c]; },
                            [&](int c) { return s_cnt[R::C_LABEL][c]; });
        if (a.stats) {
            a.stats[R::S_LOSS] = st[0], a.stats[R::S_ACCURACY] = st[1], a.stats[R::S_F1] = st[2];
            a.stats[R::S_OOD_LOSS_SUM] = (float)ood_loss, a.stats[R::S_OOD_CORRECT] = (float)ood_correct;
            a.stats[R::S_OOD_ROWS] = (float)ood_rows, a.stats[R::S_ROWS] = (float)M, a.stats[R::S_BAD] = (float)bad;
        }
    }
    if (a.train) {
        a.counts[2] += bad;
        if (M > 0) {
            const double pow1 = a.beta_pow[0] * a.beta1, pow2 = a.beta_pow[1] * a.beta2;
            a.beta_pow[0] = pow1, a.beta_pow[1] = pow2;
            a.step[0] = a.step[0] + 1;
            const P::StepScalars s = R::step_scalars(pow1, pow2);
            a.scal[0] = 1.f, a.scal[1] = s.coef, a.scal[2] = s.bc1, a.scal[3] = s.rbc2;
            a.counts[0] += 1;
            for (int k = 0; k < 3; k++) a.sums[k] += (double)st[k];
        } else {
            a.scal[0] = 0.f;
            a.counts[1] += 1;
        }
    } else {
        // acc: 4 float64 (loss, accuracy, F1, OOD loss sums), then int32: batches, skipped, ood_correct, ood_rows, bad, 3 unused, and
        // the three OOD per-class counters
        double *__restrict__ ad = reinterpret_cast<double *>(a.acc);
        int *__restrict__ ai = a.acc + 8;
        ai[4] += bad;
        if (M > 0) {
            for (int k = 0; k < 3; k++) ad[k] += (double)st[k];
            ad[3] += ood_loss;
            ai[0] += 1, ai[2] += ood_correct, ai[3] += ood_rows;
            for (int k = 0; k < 3; k++)
                for (int c = 0; c < R::CLASSES; c++) ai[8 + k * R::CLASSES + c] += s_cnt[R::C_OOD_TP + k][c];
        } else {
            ai[1] += 1;
        }
    }
}

__global__ __launch_bounds__(NT) void k_lp_adamw(int K, P::AdamCoefs c, float weight_decay, const float *__restrict__ lr,
                                                 const float *__restrict__ scal, const float *__restrict__ grad,
                                                 float *__restrict__ weight, float *__restrict__ exp_avg,
                                                 float *__restrict__ exp_avg_sq, float *__restrict__ packed) {
    const int e = blockIdx.x * NT + threadIdx.x;
    if (e >= F * K + F || scal[0] == 0.f) return;  // M == 0: the reference's `continue`
    const P::StepScalars s{0.f, scal[1], scal[2], scal[3]};
    const float rate = lr[0];
    float p = weight[e], m = exp_avg[e], v = exp_avg_sq[e];
    R::O::adamw(c, s, rate, R::O::decay_of(rate, weight_decay), grad[e], p, m, v);
    weight[e] = p, exp_avg[e] = m, exp_avg_sq[e] = v;
    packed[e < F * K ? packed_at(e / K, e % K) : W64 + (e - F * K)] = p;
}

// the chunk's tokens up to the output of layer `layer` of the tapped block (-1: its last), in X
void launch_tap(const gd_bc_policy &p, hipStream_t st, const float *obs, const unsigned char *pm, const unsigned char *rm, int r0,
                int rows, int tap, float *X, float *Kb, float *Vb, int layer = -1) {
    const BCDims d = bc_dims(p);
    launch_bc_embed(p, 64, st, obs + (size_t)r0 * d.R * d.D, rows, X);
    const int layers = layer < 0 ? p.fusion_layers + (tap == GD_LP_TAP_RO ? p.branch_layers : 0) : bc_tap_layer(p, tap, layer) + 1;
    for (int i = 0; i < layers; i++)
        launch_bc_self_layer(p, 64, st, pm + (size_t)r0 * d.R * (d.A - 1), rm + (size_t)r0 * d.R * ROADS, rows, i, X, Kb, Vb, nullptr, nullptr);
}

}  // namespace

void launch_bc_hidden(const gd_bc_policy &p, hipStream_t st, const float *obs, const unsigned char *partner_mask,
                      const unsigned char *road_mask, int n, int tap, float *out, int layer) {
    const BCDims d = bc_dims(p);
    const size_t per = (size_t)p.chunk_rows * d.L * F;
    float *X = p.scratch, *Kb = p.scratch + per, *Vb = p.scratch + 2 * per;
    for (int r0 = 0; r0 < n; r0 += p.chunk_rows) {
        const int rows = std::min(p.chunk_rows, n - r0);
        launch_tap(p, st, obs, partner_mask, road_mask, r0, rows, tap, X, Kb, Vb, layer);
        hipLaunchKernelGGL(k_lp_copy, dim3((unsigned)((d.A * 16 + 255) / 256), (unsigned)rows), dim3(256), 0, st, d.A, d.L, r0, X, out);
    }
}

// mode 0: logits and / or pred only; 1: one gradient step; 2: one batch of the evaluation added to acc
void launch_lp(const gd_bc_policy *p, const gd_lp_probe &lp, hipStream_t st, const float *obs, const unsigned char *partner_mask,
               const unsigned char *road_mask, int n, const unsigned char *mask, const int64_t *labels, const gd_lp_rows *rows_out,
               int mode, int *acc) {
    const int K = lp.in_features, P_ = lp.num_partials, GF = F * K + F;
    LPArgs a{};
    a.exp = lp.exp, a.model = lp.model, a.K = K, a.A = lp.max_agents, a.Rs = lp.num_stack;
    a.D = EGO_K + PARTNER_K * (a.A - 1) + ROAD_K * ROADS, a.L = a.A + ROADS;
    a.stats = mode != 0, a.want_grad = mode == 1;
    a.packed = lp.packed, a.mask = mask, a.labels = labels;
    if (rows_out) a.logits = rows_out->logits, a.loss_row = rows_out->loss_row, a.pred = rows_out->pred;
    if (mode != 0) {
        a.part_f = lp.part_f, a.part_d = lp.part_d, a.part_i = lp.part_i;
        hipLaunchKernelGGL(k_lp_zero, dim3(64), dim3(256), 0, st, lp.part_f, (long long)P_ * GF, lp.part_d,
                           (long long)P_ * R::PART_DOUBLES, lp.part_i, (long long)P_ * R::PART_INTS);
    }
    if (lp.model == GD_LP_BASELINE) {
        a.r0 = 0, a.rows = n, a.obs = obs;
        hipLaunchKernelGGL(k_lp_rows<true>, dim3((unsigned)P_), dim3(64), 0, st, a);
    } else {
        const size_t per = (size_t)p->chunk_rows * a.L * F;
        float *X = p->scratch, *Kb = p->scratch + per, *Vb = p->scratch + 2 * per;
        a.X = X;
        const int tap = lp.model == GD_LP_EARLY ? GD_LP_TAP_FUSION : GD_LP_TAP_RO;
        for (int r0 = 0; r0 < n; r0 += p->chunk_rows) {
            a.r0 = r0, a.rows = std::min(p->chunk_rows, n - r0);
            launch_tap(*p, st, obs, partner_mask, road_mask, r0, a.rows, tap, X, Kb, Vb);
            hipLaunchKernelGGL(k_lp_rows<false>, dim3((unsigned)P_), dim3(64), 0, st, a);
        }
    }
    if (mode == 0) return;
    LPReduce r{};
    r.P = P_, r.K = K, r.train = mode == 1, r.beta1 = lp.beta1, r.beta2 = lp.beta2;
    r.part_f = lp.part_f, r.part_d = lp.part_d, r.part_i = lp.part_i;
    r.grad = mode == 1 ? lp.grad : nullptr, r.stats = lp.stats, r.scal = lp.scal, r.sums = lp.sums, r.beta_pow = lp.beta_pow;
    r.counts = lp.counts, r.step = lp.step, r.acc = acc;
    const unsigned blocks = (unsigned)((GF + NT - 1) / NT);
    hipLaunchKernelGGL(k_lp_reduce, dim3(mode == 1 ? blocks : 1u), dim3(NT), 0, st, r);
    if (mode == 1)
        hipLaunchKernelGGL(k_lp_adamw, dim3(blocks), dim3(NT), 0, st, K, P::adam_coefs(lp.beta1, lp.beta2, lp.eps), lp.weight_decay, lp.lr,
                           lp.scal, lp.grad, lp.weight, lp.exp_avg, lp.exp_avg_sq, lp.packed);
}

}  // namespace gd
