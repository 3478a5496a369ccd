// The bookkeeping of the closed-loop PPO evaluator (policy_rollout.hip) as plain C++, so that the device and a host program
// (tests/policy_rollout_rule_host.cpp) run the same arithmetic.  It restates the metrics of the reference's evaluation rollout
// (examples/experimental/eval_utils.py rollout(), lines 105-112, 157-179, 190-212):
//     row step:   a row that was live BEFORE step t adds the info row read after it: off_road += info[0], collided += info[1] +
//                 info[2], goal_achieved += info[3] (raw float32 sums, never clamped: eval_utils.py:162-164); then
//                 live &= !done (:167)
//     world test: the number of mask slots whose done flag is set NOW equals the world's number of mask slots (:170-174) -- a
//                 world without a mask slot passes at t = 0; a done flag on a slot outside the mask does not count.  The first
//                 t at which a still-active world passes is its episode length, and the world becomes inactive (:176-179)
//     counts:     per world the rows whose accumulator is > 0 (goal_achieved, collided, off_road) and the rows with all three
//                 == 0 (other), as float32; controlled = the world's rows; the four fractions count / controlled, NaN (0 / 0)
//                 for a world without rows (:191-212)
//     summary:    [goal_achieved, collided, off_road, other (the four counts summed over the worlds), n_rows (controlled summed),
//                 worlds_with_rows, iterations (the t < n_steps whose any_active[t] is set), mean_episode_length (the episode
//                 lengths summed / the number of worlds)]
// Everything is float32 without contraction.  The summary's sums have one fixed order: lane l of LANES adds worlds l, l + LANES,
// ... in ascending order, then the lanes' partial sums are added in ascending lane order (every addend is a whole number, so
// below 2^24 the sums are exact in any order; the order is fixed all the same).
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define GD_PR_FN __host__ __device__ __forceinline__
#else
#define GD_PR_FN inline
#endif

namespace gd {
namespace policy_rollout_rule {

constexpr int LANES = 256;
constexpr int SUMMARY = 8;
enum { S_GOAL_ACHIEVED, S_COLLIDED, S_OFF_ROAD, S_OTHER, S_N_ROWS, S_WORLDS_WITH_ROWS, S_ITERATIONS, S_MEAN_EPISODE_LENGTH };
constexpr int PARTIALS = 7;  // per lane: the four counts, controlled, worlds with rows, episode lengths

struct Row {
    uint8_t live;
    float goal_achieved, collided, off_road;
};

GD_PR_FN Row fresh() { return Row{1, 0.f, 0.f, 0.f}; }

// done, info (off_road, collided with a vehicle, collided with a non-vehicle, goal_achieved, type): read AFTER step t
GD_PR_FN void row_step(Row &r, int32_t done, const int32_t *info) {
    if (r.live) {
        r.off_road = r.off_road + (float)info[0];
        r.collided = r.collided + (float)(info[1] + info[2]);
        r.goal_achieved = r.goal_achieved + (float)info[3];
    }
    r.live = (r.live && done == 0) ? 1 : 0;
}

// mask slots of the world whose done flag is set now, against all of its mask slots
GD_PR_FN bool world_done(int done_mask_slots, int mask_slots) { return done_mask_slots == mask_slots; }

// what a row adds to its world's counts: bit 0 goal_achieved, 1 collided, 2 off_road, 3 other
enum { F_GOAL = 1, F_COLLIDED = 2, F_OFF_ROAD = 4, F_OTHER = 8 };
GD_PR_FN int row_flags(const Row &r) {
    int f = 0;
    if (r.goal_achieved > 0.f) f |= F_GOAL;
    if (r.collided > 0.f) f |= F_COLLIDED;
    if (r.off_road > 0.f) f |= F_OFF_ROAD;
    if (r.goal_achieved == 0.f && r.collided == 0.f && r.off_road == 0.f) f |= F_OTHER;
    return f;
}

struct World {
    float goal_achieved_count, frac_goal_achieved, collided_count, frac_collided, off_road_count, frac_off_road, other_count,
        frac_other, controlled;
};

GD_PR_FN World world_counts(int goal, int collided, int off_road, int other, int controlled) {
    World w;
    w.controlled = (float)controlled;
    w.goal_achieved_count = (float)goal, w.collided_count = (float)collided;
    w.off_road_count = (float)off_road, w.other_count = (float)other;
    w.frac_goal_achieved = w.goal_achieved_count / w.controlled;  // (0 / 0 = NaN for a world without rows: kept)
    w.frac_collided = w.collided_count / w.controlled;
    w.frac_off_road = w.off_road_count / w.controlled;
    w.frac_other = w.other_count / w.controlled;
    return w;
}

// one lane's partial sums over its worlds: p[0..PARTIALS)
GD_PR_FN void lane_sums(int lane, int n_worlds, const float *goal, const float *collided, const float *off_road, const float *other,
                        const float *controlled, const float *episode_lengths, float *p) {
    for (int k = 0; k < PARTIALS; k++) p[k] = 0.f;
    for (int w = lane; w < n_worlds; w += LANES) {
        p[0] = p[0] + goal[w];
        p[1] = p[1] + collided[w];
        p[2] = p[2] + off_road[w];
        p[3] = p[3] + other[w];
        p[4] = p[4] + controlled[w];
        p[5] = p[5] + (controlled[w] > 0.f ? 1.f : 0.f);
        p[6] = p[6] + episode_lengths[w];
    }
}

// partials [LANES][PARTIALS]; any_active [n_steps] the iterations that exist
GD_PR_FN void finish(const float *partials, int n_worlds, const int32_t *any_active, int n_steps, float *out) {
    float s[PARTIALS];
    for (int k = 0; k < PARTIALS; k++) s[k] = 0.f;
    for (int l = 0; l < LANES; l++)
        for (int k = 0; k < PARTIALS; k++) s[k] = s[k] + partials[l * PARTIALS + k];
    int iterations = 0;
    for (int t = 0; t < n_steps; t++) iterations += any_active[t] != 0 ? 1 : 0;
    out[S_GOAL_ACHIEVED] = s[0];
    out[S_COLLIDED] = s[1];
    out[S_OFF_ROAD] = s[2];
    out[S_OTHER] = s[3];
    out[S_N_ROWS] = s[4];
    out[S_WORLDS_WITH_ROWS] = s[5];
    out[S_ITERATIONS] = (float)iterations;
    out[S_MEAN_EPISODE_LENGTH] = s[6] / (float)n_worlds;
}

}  // namespace policy_rollout_rule
}  // namespace gd
