// The arithmetic of the multi-policy evaluator (gd_owned_rows, gd_policy_forward_owned, gd_multi_policy_rollout) as plain C++,
// so that the device and a host program (tests/multi_policy_rule_host.cpp) run the same code.
//     segments:   the owned row list has one segment per policy.  start[0] = 0 and start[p + 1] = round_up(start[p] + count[p],
//                 SEGMENT_ALIGN): every segment starts at a multiple of 32, the rows of k_policy_tail's one wave, so a wave
//                 of either forward kernel reads ONE policy's weights.  Position q belongs to the segment p with
//                 start[p] <= q < start[p] + count[p]; the positions between a segment's end and the next start are padding.
//     counts:     the reference's compute_metrics (gpudrive/utils/multi_policy_rollout.py:156-169): per policy and world the
//                 rows of the policy whose accumulator is > 0, as float32, and the three fractions count / denominator, where
//                 the denominator is the reference's controlled_per_scene -- the sum over ALL policies of mask.sum(dim=1), one
//                 number per world, not per policy.  0 / 0 is NaN and is kept; a denominator above the number of rows is the
//                 caller's business.
//     summary:    per policy [goal_achieved, collided, off_road (the three counts summed over the worlds), n_rows (the
//                 policy's rows summed over the worlds)], in policy_rollout_rule.hpp's fixed order: lane l of LANES adds worlds
//                 l, l + LANES, ... ascending, then the lanes' partial sums are added in ascending lane order.
// Everything is float32 without contraction.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define GD_MP_FN __host__ __device__ __forceinline__
#else
#define GD_MP_FN inline
#endif

namespace gd {
namespace multi_policy_rule {

constexpr int MAX_POLICIES = 8;    // GD_POLICY_SET_MAX
constexpr int SEGMENT_ALIGN = 32;  // the rows of one wave of k_policy_tail
constexpr int LANES = 256;
constexpr int SUMMARY = 4;  // per policy
enum { S_GOAL_ACHIEVED, S_COLLIDED, S_OFF_ROAD, S_N_ROWS };

GD_MP_FN int round_up(int v) { return (v + SEGMENT_ALIGN - 1) / SEGMENT_ALIGN * SEGMENT_ALIGN; }

// start[0 .. n_policies] from count[0 .. n_policies)
GD_MP_FN void segment_starts(int n_policies, const int32_t *count, int32_t *start) {
    start[0] = 0;
    for (int p = 0; p < n_policies; p++) start[p + 1] = round_up(start[p] + count[p]);
}

// the positions the list's arrays hold: n rows and up to SEGMENT_ALIGN - 1 of padding per segment
GD_MP_FN int list_positions(int n, int n_policies) { return n + SEGMENT_ALIGN * n_policies; }

// The segment of position q, or -1 for padding and for positions past the last segment.  `limit` is the size of the list's
// arrays: whatever start and count hold, a position with a segment is inside [0, limit).
GD_MP_FN int segment_of(int q, int n_policies, const int32_t *start, const int32_t *count, int limit) {
    if (q < 0 || q >= limit) return -1;
    int seg = -1;
    for (int p = 0; p < n_policies; p++) {
        const int s = start[p], c = count[p];
        if (c > 0 && s >= 0 && q >= s && q - s < c) seg = p;
    }
    return seg;
}

struct World {
    float goal_achieved_count, frac_goal_achieved, collided_count, frac_collided, off_road_count, frac_off_road, n_rows;
};

GD_MP_FN World world_counts(int goal, int collided, int off_road, int rows, float denominator) {
    World w;
    w.goal_achieved_count = (float)goal, w.collided_count = (float)collided, w.off_road_count = (float)off_road;
    w.n_rows = (float)rows;
    w.frac_goal_achieved = w.goal_achieved_count / denominator;  // (0 / 0 = NaN: kept)
    w.frac_collided = w.collided_count / denominator;
    w.frac_off_road = w.off_road_count / denominator;
    return w;
}

// one lane's partial sums over its worlds of one policy: p[0 .. SUMMARY)
GD_MP_FN void lane_sums(int lane, int n_worlds, const float *goal, const float *collided, const float *off_road, const float *rows,
                        float *p) {
    for (int k = 0; k < SUMMARY; k++) p[k] = 0.f;
    for (int w = lane; w < n_worlds; w += LANES) {
        p[S_GOAL_ACHIEVED] = p[S_GOAL_ACHIEVED] + goal[w];
        p[S_COLLIDED] = p[S_COLLIDED] + collided[w];
        p[S_OFF_ROAD] = p[S_OFF_ROAD] + off_road[w];
        p[S_N_ROWS] = p[S_N_ROWS] + rows[w];
    }
}

// partials [LANES][SUMMARY] of one policy -> out[0 .. SUMMARY)
GD_MP_FN void finish(const float *partials, float *out) {
    for (int k = 0; k < SUMMARY; k++) out[k] = 0.f;
    for (int l = 0; l < LANES; l++)
        for (int k = 0; k < SUMMARY; k++) out[k] = out[k] + partials[l * SUMMARY + k];
}

}  // namespace multi_policy_rule
}  // namespace gd
