// Closed-loop PPO evaluator (gd_policy_rollout): the reference's evaluation rollout (examples/experimental/eval_utils.py
// rollout(), lines 94-227) between the steps of one episode, with gd_policy_forward as the policy.  Per time index t the
// engine launches
//   gd_policy_forward   all N learner rows of the attached [N][D] buffer -> actions (dead rows too: there is no compaction);
//                       its own three launches
//   k_pr_actions(t)     a lane per agent slot of the W * A: action columns 0..2 = table[index] for a live row, table[0] for
//                       every other slot (the reference scatters into a zero INDEX template and decodes it, eval_utils.py:
//                       125-131); a live row's index outside the table leaves the action as it was; the optional records
//                       actions_idx / live_mask
//   the step
//   k_pr_book(t)        one workgroup per world, a lane per slot: rule.hpp's row step (the sums of rows live before the step,
//                       live &= !done), the world test by wave ballot and LDS, episode_lengths, any_active[t + 1] (the same
//                       value from every world still active: a plain store), the indices outside the table counted per
//                       world, the optional record agent_positions
// so 2 launches per step beside the forward's three and the step's.  Both kernels return at once when iteration t does not
// exist (any_active[t] == 0, the reference's `break`) -- the action kernel after writing the actions, which are table[0] in
// every slot by then.  After the loop k_pr_world (a workgroup per world: counts and fractions) and k_pr_summary (one
// workgroup, the fixed order of policy_rollout_rule.hpp; it also adds the counted indices to the simulator's counter with a
// plain read-modify-write by one lane: everything that touches that counter is ordered on the simulator's stream).  No atomics.
#include <hip/hip_runtime.h>

#include "engine.hpp"
#include "policy_rollout_rule.hpp"

namespace gd {

namespace {

namespace R = policy_rollout_rule;

constexpr int T = GD_EPISODE_LEN;
constexpr int MAX_WAVES = GD_MAX_AGENTS_LIMIT / 64;

__global__ __launch_bounds__(256) void k_pr_actions(DevSim d, gd_policy_rollout_buffers b, int t, int slots) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= slots) return;
    const int n = d.row_of_slot[i];
    const bool row = n >= 0 && n < b.n_rows;
    const bool live = row && b.live[n] != 0;
    const int64_t k = live ? b.actions[n] : 0;
    if (k >= 0 && k < b.n_actions) {  // (outside the table: the action stays, k_pr_book counts it)
        const float *v = b.table + k * 3;
        float *dst = d.action + (size_t)i * 10;
        dst[0] = v[0];
        dst[1] = v[1];
        dst[2] = v[2];
    }
    if (row && b.any_active[t] != 0) {
        const size_t nt = (size_t)n * T + t;
        if (b.actions_idx) b.actions_idx[nt] = live ? k : -1;
        if (b.live_mask) b.live_mask[nt] = live ? 1 : 0;
    }
}

// sums of three per-lane flags over the workgroup (A_T lanes): one ballot per flag and wave, the waves' counts through LDS
template <int A_T>
__device__ __forceinline__ void count3(bool f0, bool f1, bool f2, int (*s_cnt)[4], int *out) {
    constexpr int WAVES = A_T / 64;
    const int wave = threadIdx.x >> 6;
    const int c0 = __popcll(__ballot(f0)), c1 = __popcll(__ballot(f1)), c2 = __popcll(__ballot(f2));
    if ((threadIdx.x & 63) == 0) s_cnt[wave][0] = c0, s_cnt[wave][1] = c1, s_cnt[wave][2] = c2;
    __syncthreads();
    out[0] = out[1] = out[2] = 0;
#pragma unroll
    for (int v = 0; v < WAVES; v++) out[0] += s_cnt[v][0], out[1] += s_cnt[v][1], out[2] += s_cnt[v][2];
}

template <int A_T>
__global__ __launch_bounds__(A_T) void k_pr_book(DevSim d, gd_policy_rollout_buffers b, int t) {
    __shared__ int s_cnt[MAX_WAVES][4];
    if (b.any_active[t] == 0) return;  // iteration t does not exist (uniform over the launch)
    const int w = blockIdx.x, a = threadIdx.x;
    const size_t slot = (size_t)w * A_T + a;
    const int n = d.row_of_slot[slot];
    const bool row = n >= 0 && n < b.n_rows;
    const int32_t done = d.done[slot];
    bool bad = false;
    if (row) {
        R::Row r{b.live[n], b.goal_achieved[n], b.collided[n], b.off_road[n]};
        if (r.live) {
            const int64_t k = b.actions[n];
            bad = k < 0 || k >= b.n_actions;
        }
        R::row_step(r, done, d.info + slot * 5);
        b.live[n] = r.live;
        b.goal_achieved[n] = r.goal_achieved;
        b.collided[n] = r.collided;
        b.off_road[n] = r.off_road;
    }
    if (b.agent_positions) {
        const float *abs = d.abs_obs + slot * 14;
        float *pos = b.agent_positions + (slot * T + t) * 2;
        pos[0] = abs[0];
        pos[1] = abs[1];
    }
    int c[3];
    count3<A_T>(row && done != 0, row, bad, s_cnt, c);
    if (a == 0) {
        if (c[2]) b.bad_indices[w] += c[2];
        if (b.world_active[w] != 0) {
            if (R::world_done(c[0], c[1])) {
                b.episode_lengths[w] = (float)t;
                b.world_active[w] = 0;
            } else {
                b.any_active[t + 1] = 1;  // the same value from every world still active: a plain store, no atomic
            }
        }
    }
}

template <int A_T>
__global__ __launch_bounds__(A_T) void k_pr_world(DevSim d, gd_policy_rollout_buffers b) {
    __shared__ int s_cnt[MAX_WAVES][4];
    __shared__ int s_first[3];
    const int w = blockIdx.x, a = threadIdx.x;
    const int n = d.row_of_slot[(size_t)w * A_T + a];
    const bool row = n >= 0 && n < b.n_rows;
    int f = 0;
    if (row) f = R::row_flags(R::Row{b.live[n], b.goal_achieved[n], b.collided[n], b.off_road[n]});
    int c[3], e[3];
    count3<A_T>((f & R::F_GOAL) != 0, (f & R::F_COLLIDED) != 0, (f & R::F_OFF_ROAD) != 0, s_cnt, c);
    if (a == 0) s_first[0] = c[0], s_first[1] = c[1], s_first[2] = c[2];
    __syncthreads();  // (s_cnt is read by every lane above before it is written again)
    count3<A_T>((f & R::F_OTHER) != 0, row, false, s_cnt, e);
    if (a == 0) {
        const R::World o = R::world_counts(s_first[0], s_first[1], s_first[2], e[0], e[1]);
        b.goal_achieved_count[w] = o.goal_achieved_count, b.frac_goal_achieved[w] = o.frac_goal_achieved;
        b.collided_count[w] = o.collided_count, b.frac_collided[w] = o.frac_collided;
        b.off_road_count[w] = o.off_road_count, b.frac_off_road[w] = o.frac_off_road;
        b.other_count[w] = o.other_count, b.frac_other[w] = o.frac_other;
        b.controlled_per_scene[w] = o.controlled;
    }
}

__global__ __launch_bounds__(R::LANES) void k_pr_summary(DevSim d, gd_policy_rollout_buffers b, int n_steps) {
    __shared__ float s_part[R::LANES * R::PARTIALS];
    __shared__ int s_bad[R::LANES];
    const int tid = threadIdx.x;
    R::lane_sums(tid, d.W, b.goal_achieved_count, b.collided_count, b.off_road_count, b.other_count, b.controlled_per_scene,
                 b.episode_lengths, s_part + tid * R::PARTIALS);
    int bad = 0;
    for (int w = tid; w < d.W; w += R::LANES) bad += b.bad_indices[w];
    s_bad[tid] = bad;
    __syncthreads();
    if (tid == 0) {
        R::finish(s_part, d.W, b.any_active, n_steps, b.summary);
        unsigned long long total = 0;
        for (int l = 0; l < R::LANES; l++) total += (unsigned long long)s_bad[l];
        if (total) *d.bad_actions = *d.bad_actions + total;
    }
}

}  // namespace

void launch_policy_rollout_actions(const DevSim &d, hipStream_t st, const gd_policy_rollout_buffers &b, int t) {
    const int slots = d.W * d.A;
    hipLaunchKernelGGL(k_pr_actions, dim3((slots + 255) / 256), dim3(256), 0, st, d, b, t, slots);
}

void launch_policy_rollout_book(const DevSim &d, hipStream_t st, const gd_policy_rollout_buffers &b, int t) {
    if (d.A == 64) hipLaunchKernelGGL(k_pr_book<64>, dim3(d.W), dim3(64), 0, st, d, b, t);
    else hipLaunchKernelGGL(k_pr_book<128>, dim3(d.W), dim3(128), 0, st, d, b, t);
}

void launch_policy_rollout_finish(const DevSim &d, hipStream_t st, const gd_policy_rollout_buffers &b, int n_steps) {
    if (d.A == 64) hipLaunchKernelGGL(k_pr_world<64>, dim3(d.W), dim3(64), 0, st, d, b);
    else hipLaunchKernelGGL(k_pr_world<128>, dim3(d.W), dim3(128), 0, st, d, b);
    hipLaunchKernelGGL(k_pr_summary, dim3(1), dim3(policy_rollout_rule::LANES), 0, st, d, b, n_steps);
}

}  // namespace gd
