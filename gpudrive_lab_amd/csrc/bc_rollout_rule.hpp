// The per-row bookkeeping of the closed-loop BC driver (bc_rollout.hip) as plain C++, so that the device and a host program
// (tests/bc_rollout_rule_host.cpp) run the same arithmetic.  It restates the metrics of the reference's closed-loop script
// (baselines/il/test/simulation.py run(), lines 45-47, 56-67, 99-105, 110-136) for one controlled agent:
//     start:    the three accumulators take the info row of the reset state (simulation.py:45-47)
//     pre(t):   goal_dist = sqrtf(x * x + y * y) of the newest frame's ego columns 3 and 4, every row, dead or not
//               (simulation.py:56-58), also init_goal_dist at t = 0 (:29-30); goal_step / off_road_step = t the first time the
//               info row read before step t has goal_achieved > 0 / off_road > 0 (:61-67); both start at -1
//     post(t):  accumulators += info columns 3, 0 and 1 + 2 of the row read after step t, clamped to 1 (:99-104);
//               dead |= done (:105)
//     summary:  [off_road_rate, veh_coll_rate, goal_rate, collision_rate, goal_progress, goal_count, n_rows, iterations];
//               goal_progress = mean(1 - ratio), ratio = goal_dist / init_goal_dist, 0 where the goal was achieved (:113-114,
//               :131-136).  The division is not guarded: a zero initial distance gives what IEEE gives.
// Everything is float32 without contraction.  The summary's sums have one fixed order: lane l of LANES adds rows l, l + LANES,
// ... in ascending order, then the lanes' partial sums are added in ascending lane order (the flag sums are exact in any order
// below 2^24 rows; the progress sum is not).  The translation unit that includes this must be compiled without contraction.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define GD_BCR_FN __host__ __device__ __forceinline__
#else
#define GD_BCR_FN inline
#endif

namespace gd {
namespace bc_rollout_rule {

constexpr int LANES = 256;
constexpr int SUMMARY = 8;
enum { S_OFF_ROAD_RATE, S_VEH_COLL_RATE, S_GOAL_RATE, S_COLLISION_RATE, S_GOAL_PROGRESS, S_GOAL_COUNT, S_N_ROWS, S_ITERATIONS };

struct Row {
    uint8_t dead;
    float goal_achieved, off_road, veh_collision;
    int32_t goal_step, off_road_step;
    float init_goal_dist, goal_dist;
};

GD_BCR_FN Row fresh() { return Row{0, 0.f, 0.f, 0.f, -1, -1, 0.f, 0.f}; }

// info: the agent's five int32 columns (off_road, collided with a vehicle, collided with a non-vehicle, goal_achieved, type)
GD_BCR_FN void accumulate(Row &r, const int32_t *info) {
    r.goal_achieved = fminf(r.goal_achieved + (float)info[3], 1.f);
    r.off_road = fminf(r.off_road + (float)info[0], 1.f);
    r.veh_collision = fminf(r.veh_collision + (float)(info[1] + info[2]), 1.f);
}

GD_BCR_FN void start(Row &r, const int32_t *info) { accumulate(r, info); }

GD_BCR_FN float goal_distance(float x, float y) { return sqrtf(x * x + y * y); }

// info: the row read BEFORE step t (after step t - 1, or the reset state at t = 0)
GD_BCR_FN void pre(Row &r, int t, const int32_t *info, float x, float y) {
    r.goal_dist = goal_distance(x, y);
    if (t == 0) r.init_goal_dist = r.goal_dist;
    if (info[3] > 0 && r.goal_step == -1) r.goal_step = t;
    if (info[0] > 0 && r.off_road_step == -1) r.off_road_step = t;
}

// done, info: read AFTER step t
GD_BCR_FN void post(Row &r, int32_t done, const int32_t *info) {
    accumulate(r, info);
    r.dead = (r.dead || done != 0) ? 1 : 0;
}

GD_BCR_FN float progress(float goal_achieved, float init_goal_dist, float goal_dist) {
    const float ratio = goal_achieved != 0.f ? 0.f : goal_dist / init_goal_dist;
    return 1.f - ratio;
}

// one lane's partial sums over its rows: p[0..4) = off_road, veh_collision, goal_achieved, progress
template <class F>
GD_BCR_FN void lane_sums(int lane, int n_rows, F row, float *p) {
    p[0] = p[1] = p[2] = p[3] = 0.f;
    for (int n = lane; n < n_rows; n += LANES) {
        const Row r = row(n);
        p[0] = p[0] + r.off_road;
        p[1] = p[1] + r.veh_collision;
        p[2] = p[2] + r.goal_achieved;
        p[3] = p[3] + progress(r.goal_achieved, r.init_goal_dist, r.goal_dist);
    }
}

// partials [LANES][4]; any_alive [n_alive] the iterations that exist
GD_BCR_FN void finish(const float *partials, int n_rows, const int32_t *any_alive, int n_alive, float *out) {
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    for (int l = 0; l < LANES; l++)
        for (int k = 0; k < 4; k++) s[k] = s[k] + partials[l * 4 + k];
    int iterations = 0;
    for (int t = 0; t < n_alive; t++) iterations += any_alive[t] != 0 ? 1 : 0;
    const float n = (float)n_rows;
    out[S_OFF_ROAD_RATE] = s[0] / n;
    out[S_VEH_COLL_RATE] = s[1] / n;
    out[S_GOAL_RATE] = s[2] / n;
    out[S_COLLISION_RATE] = out[S_OFF_ROAD_RATE] + out[S_VEH_COLL_RATE];
    out[S_GOAL_PROGRESS] = s[3] / n;
    out[S_GOAL_COUNT] = s[2];
    out[S_N_ROWS] = n;
    out[S_ITERATIONS] = (float)iterations;
}

}  // namespace bc_rollout_rule
}  // namespace gd
