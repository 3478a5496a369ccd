// Expert trajectory recorder (gd_record_expert; SURVEY.md section 8f, rank 4, the second caller): the imitation-learning
// dataset that the reference's save_trajectory (gpudrive/integrations/il/storage.py:10-109) fills with a Python loop over every
// controlled agent inside a loop over 91 steps -- seven indexed tensor copies per agent and step (storage.py:47-56) -- written
// by one launch per time index between the steps of a log playback.  Launch t does, for recorded row n = blockIdx.x of agent
// slot row_slot[n]:
//   post(t - 1), t >= 1, only if some recorded row was alive before step t - 1 (any_alive[t - 1], the reference's `break`,
//       storage.py:82-89, without a host read): dead |= done (storage.py:61-63) and the three accumulators clamped to 1
//       (storage.py:73-80);
//   pre(t), t < n_steps: dead_mask[n][t] = dead (storage.py:56) and, for a live row, storage.py:49-55: the packed observation
//       (the same bits as k_pack_obs, from the same raw rows through pack_cols.hpp), the expert action of step t, the partner
//       and road masks (env_torch.py:1224-1272) and the global pose; one lane raises any_alive[t].
// Rows and steps that are not written keep what the caller filled in (storage.py:29-35).
#include <hip/hip_runtime.h>

#include "engine.hpp"
#include "expert.hpp"
#include "pack_cols.hpp"

namespace gd {

namespace {

constexpr int K = GD_MAP_OBS_K;
constexpr int T = GD_EPISODE_LEN;
constexpr int RESP_STATIC = 2;  // ResponseType::Static (env_torch.py:1236: response_type == 2)

// column j of the packed row (k_pack_obs's element, restated: that kernel's file keeps its own copy private)
template <int A_T>
__device__ __forceinline__ float record_element(const float *self, const float *partner, const float *road, int j) {
    if (j < 6) return pack_ego_col(self, j);
    if (j < 6 + (A_T - 1) * 6) {
        const int p = j - 6, k = p / 6, c = p - k * 6;
        return pack_partner_col(partner[k * 9 + c], c);
    }
    const int p = j - 6 - (A_T - 1) * 6, k = p / 13, c = p - k * 13;
    return pack_road_col(road[k * 9 + (c < 6 ? c : 6)], c);
}

template <int A_T>
__global__ __launch_bounds__(256) void k_record(DevSim d, gd_record_buffers b, int t, int pre) {
    constexpr int D = 6 + (A_T - 1) * 6 + K * 13;
    static_assert(D % 4 == 0 && (K * 9) % 4 == 0, "rows are whole float4 groups");
    constexpr int Q = D / 4, NP = (A_T - 1) * 9, NR = K * 9;
    __shared__ float s_self[8];
    __shared__ float s_partner[NP];
    __shared__ __attribute__((aligned(16))) float s_road[NR];
    const int n = blockIdx.x, tid = threadIdx.x;
    const int slot = b.row_slot[n];
    if (slot < 0 || slot >= d.W * A_T) return;  // not an agent slot: the row keeps its defaults
    bool dead = b.dead[n] != 0;
    if (t >= 1 && b.any_alive[t - 1] != 0) {  // post(t - 1): the step has run
        dead = dead || d.done[slot] != 0;
        if (tid == 0) {
            const int32_t *info = d.info + (size_t)slot * 5;
            b.dead[n] = dead ? 1 : 0;
            b.goal_achieved[n] = fminf(b.goal_achieved[n] + (float)info[3], 1.f);
            b.off_road[n] = fminf(b.off_road[n] + (float)info[0], 1.f);
            b.veh_collision[n] = fminf(b.veh_collision[n] + (float)(info[1] + info[2]), 1.f);
        }
    }
    if (!pre) return;
    const size_t nt = (size_t)n * T + t;
    if (tid == 0) b.dead_mask[nt] = dead ? 1 : 0;
    if (dead) return;  // (uniform over the workgroup)
    if (tid == 0) b.any_alive[t] = 1;  // the same value from every live row's workgroup: a plain store, no atomic

    const size_t agent = (size_t)slot;
    if (tid < 8) s_self[tid] = d.self_obs[agent * 8 + tid];
    for (int i = tid; i < NP; i += 256) s_partner[i] = d.partner[agent * NP + i];
    const float4 *rsrc = reinterpret_cast<const float4 *>(d.agent_map + agent * NR);
    for (int i = tid; i < NR / 4; i += 256) reinterpret_cast<float4 *>(s_road)[i] = rsrc[i];
    __syncthreads();

    typedef float f4 __attribute__((ext_vector_type(4)));
    f4 *orow = reinterpret_cast<f4 *>(b.obs + nt * D);  // D * 4 bytes is a multiple of 16: every (n, t) row is 16-byte aligned
    for (int q = tid; q < Q; q += 256) {
        const f4 v = {record_element<A_T>(s_self, s_partner, s_road, 4 * q + 0), record_element<A_T>(s_self, s_partner, s_road, 4 * q + 1),
                      record_element<A_T>(s_self, s_partner, s_road, 4 * q + 2), record_element<A_T>(s_self, s_partner, s_road, 4 * q + 3)};
        __builtin_nontemporal_store(v, orow + q);  // written once, read by the host much later
    }

    // partner j of ego slot a is agent slot j for j < a, j + 1 otherwise (the rows of ~eye(A), harness.py:197-198)
    const int w = slot / A_T, a = slot - w * A_T;
    for (int j = tid; j < A_T - 1; j += 256) {
        const float *p = s_partner + j * 9;
        float sum = pack_partner_col(p[0], 0);
#pragma unroll
        for (int c = 1; c < 6; c++) sum = sum + pack_partner_col(p[c], c);  // left to right, fp32 (the build never contracts)
        const bool is_static = d.resp_export[w * A_T + (j < a ? j : j + 1)] == RESP_STATIC;
        b.partner_mask[nt * (A_T - 1) + j] = (is_static && sum != 0.f) ? 1 : (p[8] <= -1.f ? 2 : 0);
    }
    for (int k = tid; k < K; k += 256) b.road_mask[nt * K + k] = s_road[k * 9 + 7] == -1.f ? 1 : 0;
    if (tid == 192) {  // (a wave the short loops above leave idle)
        // never the State model (the engine refuses it): with its branch ruled out, act[] stays in registers
        const int model = d.p.dynamicsModel == GD_DYNAMICS_DELTA_LOCAL ? GD_DYNAMICS_DELTA_LOCAL : GD_DYNAMICS_CLASSIC;
        float act[10];
        expert_action(d.traj + agent * GD_TRAJECTORY_FLOATS, t, model, act);
        b.actions[nt * 3 + 0] = act[0];
        b.actions[nt * 3 + 1] = act[1];
        b.actions[nt * 3 + 2] = act[2];
        const float *abs = d.abs_obs + agent * 14;
        b.ego_global_pos[nt * 2 + 0] = abs[0];
        b.ego_global_pos[nt * 2 + 1] = abs[1];
        b.ego_global_rot[nt] = abs[7];
    }
}

}  // namespace

void launch_record(const DevSim &d, hipStream_t st, const gd_record_buffers &b, int t, bool pre) {
    if (b.n_rows == 0) return;
    if (d.A == 64) hipLaunchKernelGGL(k_record<64>, dim3(b.n_rows), dim3(256), 0, st, d, b, t, pre ? 1 : 0);
    else hipLaunchKernelGGL(k_record<128>, dim3(b.n_rows), dim3(256), 0, st, d, b, t, pre ? 1 : 0);
}

}  // namespace gd
