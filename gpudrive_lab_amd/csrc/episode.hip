// Episode bookkeeping on the device: what PufferGPUDrive.step() does
// with ~25 torch ops, two host synchronisations (`.item()`, `.cpu().numpy()`) and a host-driven reset
// per step (reference gpudrive/env/env_puffer.py:250-403; rewards gpudrive/env/env_torch.py:469-505;
// Info columns gpudrive/datatypes/info.py:11-15), as one kernel per step:
//
//   reward   = collision_w * (info[1] + info[2]) + goal_w * info[3] + off_road_w * info[0]
//              (weighted_combination) or the simulator's reward (sparse_on_goal_achieved);
//              reward_conditioned: the same sum with the agent slot's own weights (reward_weights[w][a][0..3));
//              distance_to_logs: the weighted sum + log_distance_weight * exp(-|log_pos[t] - pos|) (gpudrive_amd.h)
//   terminal = done != 0
//   returns[live] += reward;  lengths += 1;  offroad += info[0];  collided += info[1] + info[2]
//   mask     = live (before the update);  live[terminal] = 0
//   truncated = !offroad && !collided && !goal_achieved
//   world done <=> every controlled agent is terminal: its episode sums go to `stats`, its trackers are
//   zeroed, live <- controlled, and its reset flag is raised ON THE DEVICE; the reset pass that follows
//   (gd_sim::reset_flagged) is launched unconditionally and returns at once when nothing was flagged.
//   reward_conditioned: a finished world's weights are redrawn here, before the reset pass (env_puffer.py:375-390), so the
//   observation of the reset world already carries them.
// One workgroup per world, one thread per agent slot.
//
// Weight draws (reference env_torch.py:247-401).  random: torch.rand cannot be matched value for value, so the draw is a
// counter-based hash instead -- key (seed, world, weight_draws[world]), counter (slot, component) -- and matches the reference
// in distribution only; it is reproducible, independent of launch order and restated bit for bit in numpy
// (tests/test_reward_modes.py).  x = upper 32 bits of the 64-bit hash, u = (x >> 8) * 2^-24 in [0, 1), and
// w = lb + u * f32(ub - lb) in f32, as the reference's `lower_bounds + random_values * bounds_range`.  preset / fixed: the
// three weights of the config, resolved on the host.
#include <hip/hip_runtime.h>

#include "engine.hpp"

namespace gd {

namespace {

__device__ __forceinline__ uint64_t mix64(uint64_t z) {  // the splitmix64 finaliser
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// draw `k` of the three weights of slot `a` of world `w` into wt[0..3)
__device__ __forceinline__ void draw_weights(const gd_episode_config &c, int w, int k, int a, float *wt) {
    const uint64_t key = mix64(c.seed ^ mix64((uint64_t)(uint32_t)w << 32 | (uint32_t)k));
#pragma unroll
    for (int j = 0; j < 3; j++) {
        float v = c.weights[j];
        if (c.condition_mode == GD_CONDITION_RANDOM) {
            const uint64_t x = mix64(key + (uint64_t)(a * 3 + j + 1) * 0x9E3779B97F4A7C15ull);
            const float u = (float)(uint32_t)(x >> 40) * 0x1p-24f;
            const float range = c.ub[j] - c.lb[j];
            v = c.lb[j] + u * range;
        }
        wt[j] = v;
    }
}

template <int A_T>
__device__ __forceinline__ float block_sum(float v, float *scratch, int a) {
    // deterministic tree reduction (the statistics are compared bit for bit against the oracle per world)
    scratch[a] = v;
    __syncthreads();
#pragma unroll
    for (int s = A_T / 2; s > 0; s >>= 1) {
        if (a < s) scratch[a] += scratch[a + s];
        __syncthreads();
    }
    const float r = scratch[0];
    __syncthreads();
    return r;
}

// weight columns 6..8 of slot i's conditioned learner row (gd_attach_packed_rows_conditioned), if it has one: a redraw reaches
// every row at once -- also the rows of padding and Static slots, whose heads no step rewrites
template <int A_T>
__device__ __forceinline__ void cond_row_weights(const DevSim &d, size_t i, const float *wt) {
    constexpr int R = 6 + (A_T - 1) * 6 + GD_MAP_OBS_K * 13 + 3;
    const int r = d.row_of_slot[i];
    if (r < 0) return;
    float *o = d.pack + (size_t)r * R + 6;
    o[0] = wt[0]; o[1] = wt[1]; o[2] = wt[2];
}

// COND: conditioned learner rows are attached with b.reward_weights as their weights; the redraw rewrites their weight columns
template <int A_T, bool COND = false>
__global__ __launch_bounds__(A_T) void k_episode_step(DevSim d, gd_episode_config c, gd_episode_buffers b) {
    const int w = blockIdx.x, a = threadIdx.x;
    const size_t i = (size_t)w * A_T + a;
    __shared__ float scratch[A_T];

    const int32_t *info = d.info + i * 5;
    const float off_road = (float)info[0];
    const float collided = (float)(info[1] + info[2]);
    const float goal = (float)info[3];
    float reward;
    if (c.reward_type == GD_EPISODE_REWARD_SPARSE) {
        reward = d.reward[i];
    } else if (c.reward_type == GD_EPISODE_REWARD_CONDITIONED) {
        const float *wt = b.reward_weights + i * 3;
        reward = (wt[0] * collided + wt[1] * goal) + wt[2] * off_road;
    } else {
        reward = (c.collision_weight * collided + c.goal_achieved_weight * goal) + c.off_road_weight * off_road;
        if (c.reward_type == GD_EPISODE_REWARD_LOG_DISTANCE) {
            // slot 0's length before this step's increment (read before the barriers below, written after them); the clamp
            // only guards the index
            const int t = min(max((int)b.episode_lengths[(size_t)w * A_T], 0), GD_EPISODE_LEN - 1);
            const float *tr = d.traj + i * GD_TRAJECTORY_FLOATS;
            const float dx = tr[2 * t] - d.abs_obs[i * 14 + 0];
            const float dy = tr[2 * t + 1] - d.abs_obs[i * 14 + 1];
            reward = reward + c.log_distance_weight * expf(-sqrtf(dx * dx + dy * dy));
        }
    }
    const bool terminal = d.done[i] != 0;
    const bool controlled = b.controlled_mask[i] != 0;
    const bool live = b.live_agent_mask[i] != 0;

    float ret = b.agent_episode_returns[i];
    if (live) ret += reward;
    const float len = b.episode_lengths[i] + 1.f;
    const float off_ep = b.offroad_in_episode[i] + off_road;
    const float col_ep = b.collided_in_episode[i] + collided;
    const bool truncated = !(off_ep != 0.f) && !(col_ep != 0.f) && !(goal != 0.f);

    b.reward_out[i] = reward;
    b.terminal_out[i] = terminal ? 1 : 0;
    b.truncated_out[i] = truncated ? 1 : 0;
    b.mask_out[i] = live ? 1 : 0;
    if (d.row_of_slot) {  // the flat outputs of the learner rows (the engine refuses them without rows)
        const int r = d.row_of_slot[i];
        if (r >= 0) {
            if (b.reward_rows) b.reward_rows[r] = reward;
            if (b.terminal_rows) b.terminal_rows[r] = terminal ? 1 : 0;
            if (b.truncated_rows) b.truncated_rows[r] = truncated ? 1 : 0;
            if (b.mask_rows) b.mask_rows[r] = live ? 1 : 0;
        }
    }

    const int n_controlled = __syncthreads_count(controlled);
    const int n_terminal = __syncthreads_count(controlled && terminal);
    const bool world_done = n_terminal == n_controlled;  // also true for a world without controlled agents
    if (world_done) {
        const bool redraw = c.reward_type == GD_EPISODE_REWARD_CONDITIONED && c.auto_reset;
        const int draw = redraw ? b.weight_draws[w] : 0;  // read before the barriers of block_sum, incremented after them
        if (redraw) {
            draw_weights(c, w, draw, a, b.reward_weights + i * 3);  // this step's reward has read the old ones
            if (COND) cond_row_weights<A_T>(d, i, b.reward_weights + i * 3);
        }
        const float fc = controlled ? 1.f : 0.f;
        float sums[8];
        sums[0] = block_sum<A_T>(fc * ret, scratch, a);
        sums[1] = block_sum<A_T>(controlled && off_ep > 0.f ? 1.f : 0.f, scratch, a);
        sums[2] = block_sum<A_T>(controlled && col_ep > 0.f ? 1.f : 0.f, scratch, a);
        sums[3] = block_sum<A_T>(fc * goal, scratch, a);
        sums[4] = block_sum<A_T>(controlled && truncated ? 1.f : 0.f, scratch, a);
        sums[5] = block_sum<A_T>(len, scratch, a);
        sums[6] = block_sum<A_T>(col_ep, scratch, a);
        sums[7] = block_sum<A_T>(off_ep, scratch, a);
        if (a == 0) {
            atomicAdd(&b.stats[GD_EPISODE_STAT_EPISODES], 1.f);
            atomicAdd(&b.stats[GD_EPISODE_STAT_FINISHED_AGENTS], (float)n_controlled);
            atomicAdd(&b.stats[GD_EPISODE_STAT_RETURN_SUM], sums[0]);
            atomicAdd(&b.stats[GD_EPISODE_STAT_OFF_ROAD_AGENTS], sums[1]);
            atomicAdd(&b.stats[GD_EPISODE_STAT_COLLIDED_AGENTS], sums[2]);
            atomicAdd(&b.stats[GD_EPISODE_STAT_GOAL_ACHIEVED], sums[3]);
            atomicAdd(&b.stats[GD_EPISODE_STAT_TRUNCATED_AGENTS], sums[4]);
            atomicAdd(&b.stats[GD_EPISODE_STAT_LENGTH_SUM], sums[5]);
            atomicAdd(&b.stats[GD_EPISODE_STAT_TOTAL_COLLISIONS], sums[6]);
            atomicAdd(&b.stats[GD_EPISODE_STAT_TOTAL_OFF_ROAD], sums[7]);
            // per-world record of the episode that just ended (deterministic, unlike the running sums)
            float *ws = b.world_stats + (size_t)w * GD_EPISODE_STATS;
            ws[GD_EPISODE_STAT_EPISODES] = 1.f;
            ws[GD_EPISODE_STAT_FINISHED_AGENTS] = (float)n_controlled;
            ws[GD_EPISODE_STAT_RETURN_SUM] = sums[0];
            ws[GD_EPISODE_STAT_OFF_ROAD_AGENTS] = sums[1];
            ws[GD_EPISODE_STAT_COLLIDED_AGENTS] = sums[2];
            ws[GD_EPISODE_STAT_GOAL_ACHIEVED] = sums[3];
            ws[GD_EPISODE_STAT_TRUNCATED_AGENTS] = sums[4];
            ws[GD_EPISODE_STAT_LENGTH_SUM] = sums[5];
            ws[GD_EPISODE_STAT_TOTAL_COLLISIONS] = sums[6];
            ws[GD_EPISODE_STAT_TOTAL_OFF_ROAD] = sums[7];
            b.done_worlds[w] = 1;
            if (c.auto_reset) { d.reset_flags[w] = 1; *d.any_reset = 1; }
            if (redraw) b.weight_draws[w] = draw + 1;
        }
        // env_puffer.py:381-391: empty the storage of the finished worlds
        b.agent_episode_returns[i] = 0.f;
        b.episode_lengths[i] = 0.f;
        b.offroad_in_episode[i] = 0.f;
        b.collided_in_episode[i] = 0.f;
        b.live_agent_mask[i] = controlled ? 1 : 0;
    } else {
        if (a == 0) b.done_worlds[w] = 0;
        b.agent_episode_returns[i] = ret;
        b.episode_lengths[i] = len;
        b.offroad_in_episode[i] = off_ep;
        b.collided_in_episode[i] = col_ep;
        b.live_agent_mask[i] = live && !terminal ? 1 : 0;
    }
}

// gd_episode_draw_weights: one workgroup per listed world (worlds == null: world blockIdx.x), one thread per agent slot
template <int A_T>
__global__ __launch_bounds__(A_T) void k_draw_weights(gd_episode_config c, gd_episode_buffers b, const int32_t *worlds) {
    const int w = worlds ? worlds[blockIdx.x] : (int)blockIdx.x, a = threadIdx.x;
    const int draw = b.weight_draws[w];
    draw_weights(c, w, draw, a, b.reward_weights + ((size_t)w * A_T + a) * 3);
    __syncthreads();
    if (a == 0) b.weight_draws[w] = draw + 1;
}

// ... while conditioned learner rows are attached with b.reward_weights as their weights: their weight columns too
template <int A_T>
__global__ __launch_bounds__(A_T) void k_draw_weights_rows(DevSim d, gd_episode_config c, gd_episode_buffers b, const int32_t *worlds) {
    const int w = worlds ? worlds[blockIdx.x] : (int)blockIdx.x, a = threadIdx.x;
    const size_t i = (size_t)w * A_T + a;
    const int draw = b.weight_draws[w];
    draw_weights(c, w, draw, a, b.reward_weights + i * 3);
    cond_row_weights<A_T>(d, i, b.reward_weights + i * 3);
    __syncthreads();
    if (a == 0) b.weight_draws[w] = draw + 1;
}

// the attached conditioned learner rows take their weights from b.reward_weights
bool cond_rows_of(const DevSim &d, const gd_episode_buffers &b) {
    return d.pack != nullptr && d.pack_rows && d.pack_weights != nullptr && d.pack_weights == b.reward_weights;
}

}  // namespace

void launch_draw_weights(const DevSim &d, hipStream_t st, const gd_episode_config &c, const gd_episode_buffers &b,
                         const int32_t *worlds, int n) {
    if (cond_rows_of(d, b)) {
        if (d.A == 64) hipLaunchKernelGGL(k_draw_weights_rows<64>, dim3(n), dim3(64), 0, st, d, c, b, worlds);
        else hipLaunchKernelGGL(k_draw_weights_rows<128>, dim3(n), dim3(128), 0, st, d, c, b, worlds);
        return;
    }
    if (d.A == 64) hipLaunchKernelGGL(k_draw_weights<64>, dim3(n), dim3(64), 0, st, c, b, worlds);
    else hipLaunchKernelGGL(k_draw_weights<128>, dim3(n), dim3(128), 0, st, c, b, worlds);
}

void launch_episode_step(const DevSim &d, hipStream_t st, const gd_episode_config &c, const gd_episode_buffers &b) {
    if (c.reward_type == GD_EPISODE_REWARD_CONDITIONED && c.auto_reset && cond_rows_of(d, b)) {
        if (d.A == 64) hipLaunchKernelGGL((k_episode_step<64, true>), dim3(d.W), dim3(64), 0, st, d, c, b);
        else hipLaunchKernelGGL((k_episode_step<128, true>), dim3(d.W), dim3(128), 0, st, d, c, b);
        return;
    }
    if (d.A == 64) hipLaunchKernelGGL(k_episode_step<64>, dim3(d.W), dim3(64), 0, st, d, c, b);
    else hipLaunchKernelGGL(k_episode_step<128>, dim3(d.W), dim3(128), 0, st, d, c, b);
}

}  // namespace gd
