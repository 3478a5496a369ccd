// Learner rows (gd_set_learner_rows, gd_set_discrete_actions): the flat, controlled-agent-only view the reference's PPO loop
// works in (gpudrive/env/env_puffer.py:235-403: obs[controlled_agent_mask], one discrete action index per controlled agent).
// The rows are the true slots of a [W][A] mask in row-major (world, agent) order -- the order torch's boolean indexing
// produces -- and the engine keeps two maps: slot -> row (-1 where the slot is not a learner row) and row -> slot.
#include <hip/hip_runtime.h>

#include "engine.hpp"

namespace gd {

namespace {

constexpr int MAP_THREADS = 1024;

// The maps, by one workgroup (a setup call, not the step path): thread t takes a contiguous chunk of the slots, counts its
// true slots, an exclusive scan over the chunk counts gives the first row of every chunk, and the chunk is walked again to
// write both maps.  `count` receives the number of rows.
__global__ __launch_bounds__(MAP_THREADS) void k_learner_rows(const uint8_t *__restrict__ mask, size_t slots, int32_t *row_of_slot,
                                                              int32_t *slot_of_row, int32_t *count) {
    __shared__ int s_scan[MAP_THREADS];
    const int t = threadIdx.x;
    const size_t chunk = (slots + MAP_THREADS - 1) / MAP_THREADS;
    const size_t b = min((size_t)t * chunk, slots), e = min(b + chunk, slots);
    int c = 0;
    for (size_t i = b; i < e; i++) c += mask[i] != 0;
    s_scan[t] = c;
    __syncthreads();
    for (int off = 1; off < MAP_THREADS; off <<= 1) {  // inclusive Hillis-Steele scan
        const int v = t >= off ? s_scan[t - off] : 0;
        __syncthreads();
        s_scan[t] += v;
        __syncthreads();
    }
    int r = s_scan[t] - c;
    for (size_t i = b; i < e; i++) {
        if (mask[i] != 0) {
            row_of_slot[i] = r;
            slot_of_row[r] = (int32_t)i;
            r++;
        } else {
            row_of_slot[i] = -1;
        }
    }
    if (t == MAP_THREADS - 1) *count = s_scan[t];
}

// _apply_actions + _copy_actions_to_simulator for a discrete action space (reference gpudrive/env/env_torch.py:615-664,
// classic / bicycle / delta_local): action[row -> slot][0..3) = table[indices[row]].  One thread per row; an index outside
// [0, n_actions) leaves the row's action as it was and is counted.
__global__ __launch_bounds__(256) void k_discrete_actions(DevSim d, const int64_t *__restrict__ indices, const float *__restrict__ table,
                                                          int n_actions) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= d.n_rows) return;
    const int64_t k = indices[r];
    if (k < 0 || k >= n_actions) {
        atomicAdd(d.bad_actions, 1ull);
        return;
    }
    float *act = d.action + (size_t)d.slot_of_row[r] * 10;
    const float *v = table + k * 3;
    act[0] = v[0];
    act[1] = v[1];
    act[2] = v[2];
}

}  // namespace

void launch_learner_rows(hipStream_t st, const uint8_t *mask, size_t slots, int32_t *row_of_slot, int32_t *slot_of_row,
                         int32_t *count) {
    hipLaunchKernelGGL(k_learner_rows, dim3(1), dim3(MAP_THREADS), 0, st, mask, slots, row_of_slot, slot_of_row, count);
}

void launch_discrete_actions(const DevSim &d, hipStream_t st, const int64_t *indices, const float *table, int n_actions) {
    if (d.n_rows == 0) return;
    hipLaunchKernelGGL(k_discrete_actions, dim3((d.n_rows + 255) / 256), dim3(256), 0, st, d, indices, table, n_actions);
}

}  // namespace gd
