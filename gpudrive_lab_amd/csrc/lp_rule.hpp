// The rule of the device linear probe (lp_probe.hip: gd_lp_forward, gd_lp_update, gd_lp_eval_accumulate) as plain C++, so that
// the device and a host program (tests/lp_rule_host.cpp) run the same arithmetic.  It is the reference's linear-probing step
// (baselines/il/linear_probing.py:169-232 and 247-310) around LinearProbPosition (gpudrive/integrations/il/linear_probing/
// lp_model.py:48-85): an nn.Linear(K, 64) on the tapped tokens, mean cross-entropy over the rows the batch's mask selects,
// accuracy, sklearn's macro F1, the same over the out-of-distribution (OOD) label subset, and torch.optim.AdamW without
// clipping, with every rounding and every order fixed.
//
// ARITHMETIC.  Everything per row and per parameter is float32 and rounds every operation (compile the including unit with
// -ffp-contract=off).  Counters are int32.  Sums over rows have float32 terms; their order is stated where they are made.
//
// ROW.  z [64] float32 are the row's logits.
//     pred     = the FIRST index of the maximum (a NaN is never greater, so a row of NaN gives 0)
//     m        = that maximum;  s = ((0 + expf(z[0] - m)) + expf(z[1] - m)) + ..  ascending;  lse = m + logf(s)
//     loss_row = lse - z[label]
//     g[c]     = expf(z[c] - m) / s - (c == label ? 1 : 0)
// expf and logf are the only transcendental steps: there the device is held to the host program within 4 float32 ulps of
// loss_row's terms (|lse| + |z[label]|) and of g, never to bits.  Everything else is bit-identical on the two sides.
//
// SELECTION.  exp 'other': the rows of sample b are its partner columns j = 0 .. A - 2 (token 1 + j), and row (b, j) is
// selected iff aux_mask[b][j] == 0 (the reference's ~future_mask).  exp 'ego': the row is sample b (token 0), selected iff
// future_valid_mask[b] != 0.  A selected row whose label lies outside [0, 63] is dropped and counted in bad_labels; its label
// is never used as an index.  M = the selected rows that are left.
//
// BATCH.  Rows are taken in tiles of 32 (for 'other' the 32 consecutive partner columns of one sample, for 'ego' 32
// consecutive samples), tiles in ascending (sample, tile) order within a chunk of chunk_rows samples, tile i of a chunk by
// partial i mod num_partials.  A partial keeps: the float32 sums of g x^T (an MFMA chain over the tile's rows, ascending, that
// continues from tile to tile) and of g (a float32 chain, ascending); the float64 sums of loss_row over all selected rows and
// over the OOD ones (ascending); the int32 counts below.  The partials are added in ascending index:
//     loss = (float) (SUM loss_row / (double) M);  accuracy = (float) ((double) correct / (double) M)
//     dW[o][i] = (SUM g[o] x[i]) / (float) M;  db[o] = (SUM g[o]) / (float) M          (float32 sums of the partials)
//     per class c: tp[c] rows with pred == label == c, np[c] rows with pred == c, nl[c] rows with label == c
//     macro F1 = the mean over the classes with np + nl > 0 of (2.0 * tp) / (double) (np + nl), in float64, ascending c,
//                rounded to float32 at the end (0 when no class qualifies).  sklearn's f1_score(average='macro'); symmetric
//                in prediction and label, so the reference's swapped call gives the same value.
// OOD: 'other' the labels x * 8 + y with x or y in {0, 1, 6, 7}; 'ego' the labels with x not in {3, 4}.  Over the selected rows
// whose label is in the set: the sum of loss_row, the correct count, the count and the three per-class counters.
//
// M == 0 is the reference's `continue`: nothing of the optimiser moves (weights, moments, step, the running products of the
// betas keep their bits), the gradient and the statistics are not written, and `skipped` advances.  The device decides it.
//
// ADAMW.  bc_opt_rule.hpp's step with coef = 1.f (the reference does not clip here): step += 1; pow1 *= beta1; pow2 *= beta2;
// bc1, rbc2 as ppo_rule::step_scalars; decay = (float) (1.0 - (double) lr * (double) weight_decay); p = p * decay; then
// ppo_rule::adam.  Bit-identical between the device and the host program.
#pragma once

#include "bc_opt_rule.hpp"

// the rule's loops over the 64 classes stay loops on the device (unrolled they cost the row kernel its registers)
#if defined(__HIPCC__)
#define GD_LP_ROLLED _Pragma("unroll 1")
#else
#define GD_LP_ROLLED
#endif

namespace gd {
namespace lp_rule {

namespace P = ppo_rule;
namespace O = bc_opt_rule;

constexpr int CLASSES = 64;
enum { EXP_OTHER = 0, EXP_EGO = 1 };
// a partial's int32 words: five counts, then six per-class counters
enum { N_CORRECT = 0, N_ROWS, N_BAD, N_OOD_CORRECT, N_OOD_ROWS, N_HEAD = 8 };
enum { C_TP = 0, C_PRED, C_LABEL, C_OOD_TP, C_OOD_PRED, C_OOD_LABEL, N_COUNTERS };
constexpr int PART_INTS = N_HEAD + N_COUNTERS * CLASSES;
constexpr int PART_DOUBLES = 2;  // SUM loss_row, SUM loss_row over the OOD rows
// gd_lp_probe.stats
enum { S_LOSS = 0, S_ACCURACY, S_F1, S_OOD_LOSS_SUM, S_OOD_CORRECT, S_OOD_ROWS, S_ROWS, S_BAD, N_STATS };

GD_PPO_FN bool selected(int exp, unsigned char mask) { return exp == EXP_OTHER ? mask == 0 : mask != 0; }
GD_PPO_FN bool label_ok(long long label) { return label >= 0 && label < CLASSES; }
GD_PPO_FN bool ood(int exp, int label) {
    const int x = label >> 3, y = label & 7;
    if (exp == EXP_OTHER) return x < 2 || x > 5 || y < 2 || y > 5;
    return x != 3 && x != 4;
}

struct Row {
    int pred;
    float m, s, lse;
};

template <class Z>
GD_PPO_FN Row row(const Z &z) {
    Row r;
    r.pred = 0, r.m = z(0);
    GD_LP_ROLLED
    for (int c = 1; c < CLASSES; c++) {
        const float v = z(c);
        if (v > r.m) r.m = v, r.pred = c;
    }
    r.s = 0.f;
    GD_LP_ROLLED
    for (int c = 0; c < CLASSES; c++) r.s = r.s + expf(z(c) - r.m);
    r.lse = r.m + logf(r.s);
    return r;
}

GD_PPO_FN float loss_row(const Row &r, float z_label) { return r.lse - z_label; }
GD_PPO_FN float grad(const Row &r, float zc, bool is_label) {
    const float p = expf(zc - r.m) / r.s;
    return is_label ? p - 1.f : p;
}

GD_PPO_FN float loss_of(double sum, int m) { return (float)(sum / (double)m); }
GD_PPO_FN float accuracy_of(int correct, int m) { return (float)((double)correct / (double)m); }
GD_PPO_FN float scaled(float sum, int m) { return sum / (float)m; }

// tp, np, nl: callables class -> count
template <class A, class B, class C>
GD_PPO_FN float macro_f1(const A &tp, const B &np, const C &nl) {
    double s = 0.0;
    int n = 0;
    for (int c = 0; c < CLASSES; c++) {
        const int d = np(c) + nl(c);
        if (d > 0) s += (2.0 * (double)tp(c)) / (double)d, n++;
    }
    return n ? (float)(s / (double)n) : 0.f;
}

// the scalars of one optimiser step from the ADVANCED running products: no clipping
GD_PPO_FN P::StepScalars step_scalars(double pow1, double pow2) {
    P::StepScalars s;
    s.total = 0.f, s.coef = 1.f;
    s.bc1 = (float)(1.0 - pow1);
    s.rbc2 = sqrtf((float)(1.0 - pow2));
    return s;
}

}  // namespace lp_rule
}  // namespace gd
