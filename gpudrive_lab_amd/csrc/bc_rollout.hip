// Closed-loop BC driver (gd_bc_rollout): the reference's closed-loop script (baselines/il/test/simulation.py run(), lines
// 22-135) between the steps of one episode, with gd_bc_forward as the policy.  Per time index t the engine launches
//   k_bc_row(t)     one workgroup per row n of agent slot row_slot[n]; nothing if iteration t does not exist (any_alive[t] == 0,
//                   the reference's `break`).  The [N][R][D] window of the row is shifted one frame in place -- every thread owns
//                   its float4 columns and walks r upwards; at t = 0 the older frames are stored as zeros, never read -- and the
//                   new packed row (the same bits as k_pack_obs, from the same raw rows through pack_cols.hpp) goes to frame
//                   R - 1; the partner value (the recorder's 0 / 1 / 2), the forward's partner mask (value == 2,
//                   simulation.py:55) and the road mask at time index R - 1; the goal distance, every row, dead or not
//                   (simulation.py:56-58); goal_step / off_road_step (simulation.py:61-67); the optional records.
//   gd_bc_forward   all N rows -> row_actions (dead rows too: there is no compaction)
//   k_bc_actions    every one of the W * A slots: a live row's action in action columns 0..2, zeros for every other slot
//                   (all_actions = zeros; all_actions[~dead] = actions, simulation.py:50, 76)
//   the step
//   k_bc_post(t)    one thread per row: the accumulators and dead |= done (simulation.py:99-105); a row that is still alive
//                   raises any_alive[t + 1] (unless t is the call's last step: iteration t + 1 is not run).  It is a launch
//                   of its own because a dead row's k_bc_row(t + 1) still moves its window and its goal distance while the
//                   iteration exists, and whether it exists depends on every other row: inside one launch that would take
//                   an atomic or a read of words other workgroups write.
// and, before t = 0, k_bc_post(-1): the accumulators take the reset state's info (simulation.py:45-47) and any_alive[0] = 1.
// gd_bc_rollout_readout (the read-outs in the loop) passes the step's slices to the forward and, without the list, launches
// k_bc_score_fill after it: 0.0 over the attention scores of the rows that were dead before the step.
// After the loop k_bc_summary: one workgroup, the fixed order of bc_rollout_rule.hpp.  No atomics anywhere.
#include <hip/hip_runtime.h>

#include "bc_rollout_rule.hpp"
#include "engine.hpp"
#include "pack_cols.hpp"

namespace gd {

namespace {

namespace R = bc_rollout_rule;

constexpr int K = GD_MAP_OBS_K;
constexpr int T = GD_EPISODE_LEN;
constexpr int RESP_STATIC = 2;  // ResponseType::Static (env_torch.py:1236: response_type == 2)

// column j of the packed row (k_pack_obs's element, restated: that kernel's file keeps its own copy private)
template <int A_T>
__device__ __forceinline__ float row_element(const float *self, const float *partner, const float *road, int j) {
    if (j < 6) return pack_ego_col(self, j);
    if (j < 6 + (A_T - 1) * 6) {
        const int p = j - 6, k = p / 6, c = p - k * 6;
        return pack_partner_col(partner[k * 9 + c], c);
    }
    const int p = j - 6 - (A_T - 1) * 6, k = p / 13, c = p - k * 13;
    return pack_road_col(road[k * 9 + (c < 6 ? c : 6)], c);
}

__device__ __forceinline__ R::Row load_row(const gd_bc_rollout_buffers &b, int n) {
    return R::Row{b.dead[n], b.goal_achieved[n], b.off_road[n], b.veh_collision[n], b.goal_step[n], b.off_road_step[n],
                  b.init_goal_dist[n], b.goal_dist[n]};
}

template <int A_T>
__global__ __launch_bounds__(256) void k_bc_row(DevSim d, gd_bc_rollout_buffers b, int t, int RS) {
    constexpr int D = 6 + (A_T - 1) * 6 + K * 13;
    static_assert(D % 4 == 0 && (K * 9) % 4 == 0, "rows are whole float4 groups");
    constexpr int Q = D / 4, NP = (A_T - 1) * 9, NR = K * 9;
    __shared__ float s_self[8];
    __shared__ float s_partner[NP];
    __shared__ __attribute__((aligned(16))) float s_road[NR];
    const int n = blockIdx.x, tid = threadIdx.x;
    if (b.any_alive[t] == 0) return;  // iteration t does not exist (uniform over the launch)
    const int slot = b.row_slot[n];
    if (slot < 0 || slot >= d.W * A_T) return;  // not an agent slot (the host refuses it; nothing is read or written)
    const bool dead = b.dead[n] != 0;

    const size_t agent = (size_t)slot;
    if (tid < 8) s_self[tid] = d.self_obs[agent * 8 + tid];
    for (int i = tid; i < NP; i += 256) s_partner[i] = d.partner[agent * NP + i];
    const float4 *rsrc = reinterpret_cast<const float4 *>(d.agent_map + agent * NR);
    for (int i = tid; i < NR / 4; i += 256) reinterpret_cast<float4 *>(s_road)[i] = rsrc[i];
    __syncthreads();

    // the window: frame r takes frame r + 1, the newest frame the packed row.  D * 4 bytes is a multiple of 16, so every
    // (n, r) frame is 16-byte aligned; thread tid owns groups tid, tid + 256, ... of every frame, so the shift is in place.
    typedef float f4 __attribute__((ext_vector_type(4)));
    f4 *win = reinterpret_cast<f4 *>(b.window + (size_t)n * RS * D);
    for (int q = tid; q < Q; q += 256) {
        if (t == 0) {
            const f4 zero = {0.f, 0.f, 0.f, 0.f};
            for (int r = 0; r + 1 < RS; r++) win[(size_t)r * Q + q] = zero;
        } else {
            for (int r = 0; r + 1 < RS; r++) win[(size_t)r * Q + q] = win[(size_t)(r + 1) * Q + q];
        }
        const f4 v = {row_element<A_T>(s_self, s_partner, s_road, 4 * q + 0), row_element<A_T>(s_self, s_partner, s_road, 4 * q + 1),
                      row_element<A_T>(s_self, s_partner, s_road, 4 * q + 2), row_element<A_T>(s_self, s_partner, s_road, 4 * q + 3)};
        win[(size_t)(RS - 1) * Q + q] = v;
    }

    // partner j of ego slot a is agent slot j for j < a, j + 1 otherwise (the rows of ~eye(A), harness.py:197-198)
    const int w = slot / A_T, a = slot - w * A_T;
    uint8_t *pm = b.partner_mask + ((size_t)n * RS + (RS - 1)) * (A_T - 1);
    for (int j = tid; j < A_T - 1; j += 256) {
        const float *p = s_partner + j * 9;
        float sum = pack_partner_col(p[0], 0);
#pragma unroll
        for (int c = 1; c < 6; c++) sum = sum + pack_partner_col(p[c], c);  // left to right, fp32 (the build never contracts)
        const bool is_static = d.resp_export[w * A_T + (j < a ? j : j + 1)] == RESP_STATIC;
        const uint8_t value = (is_static && sum != 0.f) ? 1 : (p[8] <= -1.f ? 2 : 0);
        b.partner_value[(size_t)n * (A_T - 1) + j] = value;
        pm[j] = value == 2 ? 1 : 0;
    }
    uint8_t *rm = b.road_mask + ((size_t)n * RS + (RS - 1)) * K;
    for (int k = tid; k < K; k += 256) rm[k] = s_road[k * 9 + 7] == -1.f ? 1 : 0;

    if (tid == 192) {  // (a wave the short loops above leave idle)
        R::Row r = load_row(b, n);
        R::pre(r, t, d.info + (size_t)slot * 5, pack_ego_col(s_self, 3), pack_ego_col(s_self, 4));
        b.goal_dist[n] = r.goal_dist;
        if (t == 0) b.init_goal_dist[n] = r.init_goal_dist;
        b.goal_step[n] = r.goal_step;
        b.off_road_step[n] = r.off_road_step;
        const size_t nt = (size_t)n * T + t;
        if (b.dead_mask) b.dead_mask[nt] = dead ? 1 : 0;
        if (!dead) {
            const float *abs = d.abs_obs + agent * 14;
            if (b.ego_global_pos) {
                b.ego_global_pos[nt * 2 + 0] = abs[0];
                b.ego_global_pos[nt * 2 + 1] = abs[1];
            }
            if (b.ego_global_rot) b.ego_global_rot[nt] = abs[7];
        }
    }
}

// every agent slot: a live row's action, zeros for everyone else
__global__ __launch_bounds__(256) void k_bc_actions(DevSim d, gd_bc_rollout_buffers b, int t, int slots) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= slots) return;
    const int n = b.row_of_slot[i];
    const bool row = n >= 0 && n < b.n_rows;
    const bool live = row && b.dead[n] == 0;
    float act[3] = {0.f, 0.f, 0.f};
    if (live) {
        act[0] = b.row_actions[n * 3 + 0];
        act[1] = b.row_actions[n * 3 + 1];
        act[2] = b.row_actions[n * 3 + 2];
    }
    float *dst = d.action + (size_t)i * 10;
    dst[0] = act[0];
    dst[1] = act[1];
    dst[2] = act[2];
    if (row && b.actions && b.any_alive[t] != 0) {
        float *rec = b.actions + ((size_t)n * T + t) * 3;
        rec[0] = act[0];
        rec[1] = act[1];
        rec[2] = act[2];
    }
}

// t = -1: the start (the reset state's info); t >= 0: the bookkeeping of step t, if iteration t exists
__global__ __launch_bounds__(256) void k_bc_post(DevSim d, gd_bc_rollout_buffers b, int t, int slots, int more) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= b.n_rows) return;
    if (t >= 0 && b.any_alive[t] == 0) return;
    const int slot = b.row_slot[n];
    if (slot < 0 || slot >= slots) return;
    R::Row r = load_row(b, n);
    const int32_t *info = d.info + (size_t)slot * 5;
    if (t < 0) R::start(r, info);
    else R::post(r, d.done[slot], info);
    b.dead[n] = r.dead;
    b.goal_achieved[n] = r.goal_achieved;
    b.off_road[n] = r.off_road;
    b.veh_collision[n] = r.veh_collision;
    if (more && r.dead == 0) b.any_alive[t + 1] = 1;  // the same value from every live row: a plain store, no atomic
}

// grid (N, ceil(per_row / 256)): the scores [N][per_row] of one step, 0.0 over the rows that were dead before it
__global__ __launch_bounds__(256) void k_bc_score_fill(gd_bc_rollout_buffers b, float *__restrict__ scores, int per_row) {
    const int n = blockIdx.x, i = blockIdx.y * 256 + threadIdx.x;
    if (i >= per_row || b.dead[n] == 0) return;
    scores[(size_t)n * per_row + i] = 0.f;
}

__global__ __launch_bounds__(R::LANES) void k_bc_summary(gd_bc_rollout_buffers b) {
    __shared__ float s_part[R::LANES * 4];
    const int tid = threadIdx.x;
    R::lane_sums(tid, b.n_rows, [&](int n) { return load_row(b, n); }, s_part + tid * 4);
    __syncthreads();
    if (tid == 0) R::finish(s_part, b.n_rows, b.any_alive, T, b.summary);
}

}  // namespace

void launch_bc_rollout_row(const DevSim &d, hipStream_t st, const gd_bc_rollout_buffers &b, int t, int num_stack) {
    if (d.A == 64) hipLaunchKernelGGL(k_bc_row<64>, dim3(b.n_rows), dim3(256), 0, st, d, b, t, num_stack);
    else hipLaunchKernelGGL(k_bc_row<128>, dim3(b.n_rows), dim3(256), 0, st, d, b, t, num_stack);
}

void launch_bc_rollout_actions(const DevSim &d, hipStream_t st, const gd_bc_rollout_buffers &b, int t) {
    const int slots = d.W * d.A;
    hipLaunchKernelGGL(k_bc_actions, dim3((slots + 255) / 256), dim3(256), 0, st, d, b, t, slots);
}

void launch_bc_rollout_post(const DevSim &d, hipStream_t st, const gd_bc_rollout_buffers &b, int t, bool more) {
    hipLaunchKernelGGL(k_bc_post, dim3((b.n_rows + 255) / 256), dim3(256), 0, st, d, b, t, d.W * d.A, more ? 1 : 0);
}

void launch_bc_rollout_score_fill(hipStream_t st, const gd_bc_rollout_buffers &b, float *scores, int per_row) {
    hipLaunchKernelGGL(k_bc_score_fill, dim3(b.n_rows, (per_row + 255) / 256), dim3(256), 0, st, b, scores, per_row);
}

void launch_bc_rollout_summary(hipStream_t st, const gd_bc_rollout_buffers &b) {
    hipLaunchKernelGGL(k_bc_summary, dim3(1), dim3(bc_rollout_rule::LANES), 0, st, b);
}

}  // namespace gd
