// The rule of the closed-loop probe read-outs (bc_readout.hip: gd_bc_forward_readout, gd_bc_rollout_readout) as plain C++, so
// that the device and a host program (tests/bc_readout_rule_host.cpp) run the same arithmetic.  It is what the reference's
// baselines/il/test/intervention.py reads per step from pairs of trained LinearProbPosition heads on one tapped layer:
//     other_pred      the class of every partner token under an 'other' probe
//     ego_pred        the class of the ego token under an 'ego' probe
//     ego_pred_prime  the ego class after row `label` of the paired 'other' probe's head.weight is added to the ego token
//
// CLASS.  z [64] float32 are a token's logits; the class is lp_rule::row(z).pred, the FIRST index of the maximum (a NaN is never
// greater, so a row of NaN gives 0).  It is stored as one byte, 0 .. 63.
//
// INTERVENTION.  h [64] is the ego token, w [64][64] the 'other' probe's head.weight in its natural layout, label the row's
// label.  A label in [0, 63] gives h'[k] = h[k] + w[label][k], one float32 add per feature (compile the including unit with
// -ffp-contract=off); any other label is "no intervention": h' = h bit for bit, w is not indexed, and the row counts once in
// bad_labels, however many pairs read it.  The logits of h' are the 'ego' probe's as for any other token.
//
// FILL.  A row that is not read in a step of the closed loop (it was dead before the step, or the step's iteration does not
// exist) holds NO_CLASS in every class output and 0.0 in the attention scores.
#pragma once

#include "lp_rule.hpp"

namespace gd {
namespace bc_readout_rule {

constexpr int MAX_PROBES = 8;            // per list ('other', 'ego')
constexpr unsigned char NO_CLASS = 255;  // the fill value of the class outputs

template <class Z>
GD_PPO_FN unsigned char class_of(const Z &z) {
    return (unsigned char)lp_rule::row(z).pred;
}

GD_PPO_FN bool label_ok(long long label) { return lp_rule::label_ok(label); }
// the row of w to add: never outside the matrix
GD_PPO_FN int label_row(long long label) { return label_ok(label) ? (int)label : 0; }
// feature k of the intervened token: hk = h[k], wk = w[label_row(label)][k]
GD_PPO_FN float intervened(float hk, float wk, bool ok) { return ok ? hk + wk : hk; }

}  // namespace bc_readout_rule
}  // namespace gd
