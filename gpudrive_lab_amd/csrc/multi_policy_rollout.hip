// Multi-policy closed-loop evaluator (gd_multi_policy_rollout): the reference's cross-play rollout
// (gpudrive/utils/multi_policy_rollout.py multi_policy_rollout(), lines 36-154, and compute_metrics, 156-169) on the device.
// The loop is gd_policy_rollout_compact's with the owned list for the live list (engine.cpp): per step gd_owned_rows (2
// launches), gd_policy_forward_owned (3), k_pr_actions, the step, k_pr_book -- policies own disjoint rows, so the reference's
// per-policy [W, A] accumulators are the per-row accumulators of gd_policy_rollout_buffers read through owner[N], and the
// action and bookkeeping kernels of policy_rollout.hip serve unchanged.  After the loop, and after k_pr_world / k_pr_summary:
//   k_mp_world    a workgroup per world, a lane per slot: per policy the rows of that policy in the world whose accumulator is
//                 > 0 (one ballot per flag, policy and wave; the waves' counts through LDS), the policy's rows, and the three
//                 fractions count / denominator[w] (multi_policy_rule.hpp: world_counts)
//   k_mp_summary  one workgroup: per policy the totals in the fixed order of multi_policy_rule.hpp
// No atomics.
#include <hip/hip_runtime.h>

#include "engine.hpp"
#include "multi_policy_rule.hpp"

namespace gd {

namespace {

namespace MP = multi_policy_rule;

constexpr int MAXP = GD_POLICY_SET_MAX;
constexpr int MAX_WAVES = GD_MAX_AGENTS_LIMIT / 64;

template <int A_T>
__global__ __launch_bounds__(A_T) void k_mp_world(DevSim d, gd_policy_rollout_buffers b, gd_multi_policy_buffers m, int P) {
    constexpr int WAVES = A_T / 64;
    __shared__ int s_cnt[MAXP][MAX_WAVES][4];
    const int w = blockIdx.x, a = threadIdx.x, wave = a >> 6;
    const int n = d.row_of_slot[(size_t)w * A_T + a];
    const bool row = n >= 0 && n < b.n_rows;
    int owner = -1;
    bool goal = false, collided = false, off_road = false;
    if (row) {
        owner = m.owner[n];
        goal = b.goal_achieved[n] > 0.f, collided = b.collided[n] > 0.f, off_road = b.off_road[n] > 0.f;
    }
#pragma unroll
    for (int p = 0; p < MAXP; p++)
        if (p < P) {
            const bool mine = owner == p;
            const int c0 = __popcll(__ballot(mine && goal)), c1 = __popcll(__ballot(mine && collided));
            const int c2 = __popcll(__ballot(mine && off_road)), c3 = __popcll(__ballot(mine));
            if ((a & 63) == 0) s_cnt[p][wave][0] = c0, s_cnt[p][wave][1] = c1, s_cnt[p][wave][2] = c2, s_cnt[p][wave][3] = c3;
        }
    __syncthreads();
    if (a < P) {
        int c[4] = {0, 0, 0, 0};
#pragma unroll
        for (int v = 0; v < WAVES; v++)
#pragma unroll
            for (int k = 0; k < 4; k++) c[k] += s_cnt[a][v][k];
        const MP::World o = MP::world_counts(c[0], c[1], c[2], c[3], m.denominator[w]);
        const size_t at = (size_t)a * d.W + w;
        m.goal_achieved_count[at] = o.goal_achieved_count, m.frac_goal_achieved[at] = o.frac_goal_achieved;
        m.collided_count[at] = o.collided_count, m.frac_collided[at] = o.frac_collided;
        m.off_road_count[at] = o.off_road_count, m.frac_off_road[at] = o.frac_off_road;
        m.n_rows[at] = o.n_rows;
    }
}

__global__ __launch_bounds__(MP::LANES) void k_mp_summary(int W, gd_multi_policy_buffers m, int P) {
    __shared__ float s_part[MP::LANES * MP::SUMMARY];
    const int tid = threadIdx.x;
    for (int p = 0; p < P; p++) {
        const size_t at = (size_t)p * W;
        MP::lane_sums(tid, W, m.goal_achieved_count + at, m.collided_count + at, m.off_road_count + at, m.n_rows + at,
                      s_part + tid * MP::SUMMARY);
        __syncthreads();
        if (tid == 0) MP::finish(s_part, m.summary + p * MP::SUMMARY);
        __syncthreads();  // (s_part is written again for the next policy)
    }
}

}  // namespace

void launch_multi_policy_finish(const DevSim &d, hipStream_t st, const gd_policy_rollout_buffers &b, const gd_multi_policy_buffers &m,
                                int n_policies) {
    if (d.A == 64) hipLaunchKernelGGL(k_mp_world<64>, dim3(d.W), dim3(64), 0, st, d, b, m, n_policies);
    else hipLaunchKernelGGL(k_mp_world<128>, dim3(d.W), dim3(128), 0, st, d, b, m, n_policies);
    hipLaunchKernelGGL(k_mp_summary, dim3(1), dim3(MP::LANES), 0, st, d.W, m, n_policies);
}

}  // namespace gd
