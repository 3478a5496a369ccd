// Fused observation pack: what GPUDriveTorchEnv.get_obs() assembles
// with ~20 torch ops and a clone per tensor (reference gpudrive/env/env_torch.py:756-896,1172-1216;
// normalisation in gpudrive/datatypes/observation.py:71-90,229-262, gpudrive/datatypes/roadgraph.py:
// 329-364; constants gpudrive/env/constants.py:6-21) in one pass over the exported tensors:
//   out[w][a] = ego(6) | partners (A-1) x 6 | road points 200 x 13      (norm_obs = True)
// Divisions are true IEEE divisions like torch's CPU kernels (torch's CUDA kernels multiply by the
// reciprocal of a scalar divisor, which may differ in the last bit).
#include <hip/hip_runtime.h>

#include "engine.hpp"
#include "expert.hpp"
#include "pack_cols.hpp"

namespace gd {

namespace {

#ifndef GD_PACK_PARTS
#define GD_PACK_PARTS 64  // workgroups per world of k_pack_obs: one agent slot each (4 or 16 per world measured the same within noise)
#endif
constexpr int K = GD_MAP_OBS_K;
// Per agent: the source rows (63 x 9 partner floats, 200 x 9 road floats: 9.5 KB) are staged in LDS with
// coalesced loads (16-byte loads for the road rows), then one thread per FOUR consecutive output floats
// (rows are 2984 floats, so float4 groups never straddle a row) computes from LDS and issues one 16-byte
// store: both directions of the 1.4 GB this pass moves per step at 1024 x 64 are fully coalesced.  Every
// output element costs ONE true division: numerator and divisor are selected per column first (pack_cols.hpp).
template <int A_T>
__device__ __forceinline__ float pack_element(const float *self, const float *partner, const float *road, int j) {
    if (j < 6) return pack_ego_col(self, j);
    if (j < 6 + (A_T - 1) * 6) {
        const int p = j - 6, k = p / 6, c = p - k * 6;
        return pack_partner_col(partner[k * 9 + c], c);
    }
    const int p = j - 6 - (A_T - 1) * 6, k = p / 13, c = p - k * 13;
    return pack_road_col(road[k * 9 + (c < 6 ? c : 6)], c);
}

// ROWS (gd_attach_packed_rows): one workgroup per learner row, blockIdx.x; out is [n_rows][D] and row r is slot slot_of_row[r].
// COND (gd_attach_packed_rows_conditioned, with ROWS): out is [n_rows][D + 3], the conditioned row ego 6 | the slot's 3 weights
// (DevSim::pack_weights) | partners | roads.  Its odd pitch leaves the row at any 16-byte phase: it is laid out in LDS and
// leaves through store_span (pack_cols.hpp), which writes exactly the row's own dwords.
template <int A_T, bool ROWS = false, bool COND = false>
__global__ __launch_bounds__(256) void k_pack_obs(DevSim d, float *out) {
    static_assert(ROWS || !COND, "the conditioned layout exists for the learner rows only");
    constexpr int D = 6 + (A_T - 1) * 6 + K * 13;
    static_assert(D % 4 == 0 && (K * 9) % 4 == 0, "rows are whole float4 groups");
    constexpr int Q = D / 4, NP = (A_T - 1) * 9, NR = K * 9;
    constexpr int GROUP = ROWS ? 1 : A_T / GD_PACK_PARTS;  // blockIdx.y: a part of the world's agent slots
    __shared__ float s_self[8];
    __shared__ float s_partner[NP];
    __shared__ __attribute__((aligned(16))) float s_road[NR];
    const int w = blockIdx.x, tid = threadIdx.x;
    for (int al = 0; al < GROUP; al++) {
        const size_t agent = ROWS ? (size_t)d.slot_of_row[w] : (size_t)w * A_T + blockIdx.y * GROUP + al;
        const size_t orow = ROWS ? (size_t)w : agent;
        if (tid < 8) s_self[tid] = d.self_obs[agent * 8 + tid];
        for (int t = tid; t < NP; t += 256) s_partner[t] = d.partner[agent * NP + t];
        const float4 *rsrc = reinterpret_cast<const float4 *>(d.agent_map + agent * NR);
        for (int t = tid; t < NR / 4; t += 256) reinterpret_cast<float4 *>(s_road)[t] = rsrc[t];
        __syncthreads();
        if constexpr (COND) {
            constexpr int R = D + 3;
            __shared__ float s_row[R];
            const float *wt = d.pack_weights + agent * 3;
            for (int j = tid; j < R; j += 256)
                s_row[j] = j < 6 ? pack_ego_col(s_self, j) : j < 9 ? wt[j - 6] : pack_element<A_T>(s_self, s_partner, s_road, j - 3);
            __syncthreads();
            store_span(s_row, out + orow * R, R, tid, 256);
            __syncthreads();
            continue;
        }
        for (int q = tid; q < Q; q += 256) {
            float4 v;
            v.x = pack_element<A_T>(s_self, s_partner, s_road, 4 * q + 0);
            v.y = pack_element<A_T>(s_self, s_partner, s_road, 4 * q + 1);
            v.z = pack_element<A_T>(s_self, s_partner, s_road, 4 * q + 2);
            v.w = pack_element<A_T>(s_self, s_partner, s_road, 4 * q + 3);
            typedef float f4 __attribute__((ext_vector_type(4)));
            const f4 vv = {v.x, v.y, v.z, v.w};
            __builtin_nontemporal_store(vv, reinterpret_cast<f4 *>(out + orow * D) + q);  // 782 MB written once: keep it out of the caches
        }
        __syncthreads();
    }
}

// ---- the conditioned row (gd_pack_observations_conditioned): ego(6) | weights(3) | partners | roads, R = D + 3 floats ----
// R is odd, so rows are no longer whole float4 groups; a world's block A * R is (A in {64, 128}) and starts 16-byte aligned.
// The stores stay 16-byte and coalesced by numbering the float4 groups over the world's block: agent slot a owns the groups
// whose first element lies in its row, [ceil(a R / 4), ceil((a + 1) R / 4)).  The last of them straddles into the next row
// by at most 3 floats, which are ego columns 0..2 of slot a + 1: they need that slot's self-observation row only.
template <int A_T>
__global__ __launch_bounds__(256) void k_pack_obs_cond(DevSim d, const float *__restrict__ weights, float *out) {
    constexpr int D = 6 + (A_T - 1) * 6 + K * 13, R = D + 3;
    static_assert((A_T * R) % 4 == 0 && (K * 9) % 4 == 0, "a world's block is whole float4 groups");
    constexpr int NP = (A_T - 1) * 9, NR = K * 9;
    constexpr int GROUP = A_T / GD_PACK_PARTS;
    __shared__ float s_self[8], s_next[8], s_wt[4];
    __shared__ float s_partner[NP];
    __shared__ __attribute__((aligned(16))) float s_road[NR];
    const int w = blockIdx.x, tid = threadIdx.x;
    typedef float f4 __attribute__((ext_vector_type(4)));
    f4 *wout = reinterpret_cast<f4 *>(out + (size_t)w * A_T * R);
    for (int al = 0; al < GROUP; al++) {
        const int a = blockIdx.y * GROUP + al;
        const size_t agent = (size_t)w * A_T + a;
        if (tid < 8) s_self[tid] = d.self_obs[agent * 8 + tid];
        else if (tid < 16 && a + 1 < A_T) s_next[tid - 8] = d.self_obs[(agent + 1) * 8 + tid - 8];
        else if (tid >= 16 && tid < 19) s_wt[tid - 16] = weights[agent * 3 + tid - 16];
        for (int t = tid; t < NP; t += 256) s_partner[t] = d.partner[agent * NP + t];
        const float4 *rsrc = reinterpret_cast<const float4 *>(d.agent_map + agent * NR);
        for (int t = tid; t < NR / 4; t += 256) reinterpret_cast<float4 *>(s_road)[t] = rsrc[t];
        __syncthreads();
        const int row0 = a * R, row1 = row0 + R;  // this slot's row within the world's block
        const int q0 = (row0 + 3) / 4, q1 = (row1 + 3) / 4;
        for (int q = q0 + tid; q < q1; q += 256) {
            float v[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int e = 4 * q + k;
                if (e >= row1) {
                    v[k] = pack_ego_col(s_next, e - row1);  // e - row1 < 3; never reached for the last slot (q1 * 4 == A R)
                } else {
                    const int j = e - row0;
                    v[k] = j < 6 ? pack_ego_col(s_self, j) : j < 9 ? s_wt[j - 6] : pack_element<A_T>(s_self, s_partner, s_road, j - 3);
                }
            }
            const f4 vv = {v[0], v[1], v[2], v[3]};
            __builtin_nontemporal_store(vv, wout + q);
        }
        __syncthreads();
    }
}

// The same rows from the attached direct-pack buffer ([rows][D], the only current copy with gd_attach_packed(only = 1)): one
// thread per output float4 group over all rows, the three weights inserted after column 5.  Inside a row's body (column >= 9
// and the group within the row) the four source floats are consecutive, 16-byte aligned up to a shift m = source index mod 4
// that is the same for the whole row: two aligned 16-byte loads and a select.  The few groups at a row's start and end take
// element by element.
template <int A_T>
__global__ __launch_bounds__(256) void k_pack_relayout(const float *__restrict__ src, const float *__restrict__ weights, float *out,
                                                       size_t groups) {
    constexpr int D = 6 + (A_T - 1) * 6 + K * 13, R = D + 3;
    static_assert(D % 4 == 0 && (A_T * R) % 4 == 0, "source rows and world blocks are whole float4 groups");
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= groups) return;
    const size_t e = 4 * g, r = e / R;
    const int j = (int)(e - r * R);
    float v[4];
    if (j >= 9 && j + 3 < R) {
        const size_t sidx = r * D + (j - 3);
        const float4 *s4 = reinterpret_cast<const float4 *>(src) + (sidx >> 2);
        const int m = (int)(sidx & 3);
        const float4 lo = s4[0];
        if (m == 0) {
            v[0] = lo.x; v[1] = lo.y; v[2] = lo.z; v[3] = lo.w;
        } else {
            const float4 hi = s4[1];  // holds source element sidx + 3 at least: inside the buffer
            if (m == 1) { v[0] = lo.y; v[1] = lo.z; v[2] = lo.w; v[3] = hi.x; }
            else if (m == 2) { v[0] = lo.z; v[1] = lo.w; v[2] = hi.x; v[3] = hi.y; }
            else { v[0] = lo.w; v[1] = hi.x; v[2] = hi.y; v[3] = hi.z; }
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const size_t rr = j + k >= R ? r + 1 : r;  // groups is whole, so row r + 1 exists when reached
            const int jj = j + k >= R ? j + k - R : j + k;
            v[k] = jj < 6 ? src[rr * D + jj] : jj < 9 ? weights[rr * 3 + jj - 6] : src[rr * D + jj - 3];
        }
    }
    typedef float f4 __attribute__((ext_vector_type(4)));
    const f4 vv = {v[0], v[1], v[2], v[3]};
    __builtin_nontemporal_store(vv, reinterpret_cast<f4 *>(out) + g);
}

// ---- expert-action export and log playback: the columns come from expert_action (expert.hpp) ----
constexpr int T = GD_EPISODE_LEN;

__global__ __launch_bounds__(256) void k_expert_actions(DevSim d, float *actions, float *pos, float *vel, float *yaw, int *valid) {
    const size_t n = (size_t)d.W * d.A * T;  // one thread per (world, agent, time step)
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= n) return;
    const size_t row = g / T;
    const int t = (int)(g - row * T);
    const float *tr = d.traj + row * GD_TRAJECTORY_FLOATS;
    const int model = d.p.dynamicsModel;
    if (actions) {
        float act[10];
        expert_action(tr, t, model, act);
        const int cols = model == GD_DYNAMICS_STATE ? 10 : 3;
        for (int c = 0; c < cols; c++) actions[g * cols + c] = act[c];
    }
    if (pos) { pos[g * 2] = tr[2 * t]; pos[g * 2 + 1] = tr[2 * t + 1]; }
    if (vel) { vel[g * 2] = tr[2 * T + 2 * t]; vel[g * 2 + 1] = tr[2 * T + 2 * t + 1]; }
    if (yaw) yaw[g] = tr[4 * T + t];
    if (valid) valid[g] = (int)tr[5 * T + t];  // .to(torch.int32) truncates
}

// advance_sim_with_log_playback (env_torch.py:1274-1293): step t feeds log_playback_traj[:, :, t, :]
// into action[:, :, :cols] for EVERY agent slot (env_torch.py:645-664), then steps the simulator.
__global__ __launch_bounds__(256) void k_set_log_actions(DevSim d, int t) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= d.W * d.A) return;
    const int model = d.p.dynamicsModel;
    float act[10];
    expert_action(d.traj + (size_t)g * GD_TRAJECTORY_FLOATS, t, model, act);
    const int cols = model == GD_DYNAMICS_STATE ? 10 : 3;
    for (int c = 0; c < cols; c++) d.action[(size_t)g * 10 + c] = act[c];
}

}  // namespace

void launch_pack_obs(const DevSim &d, hipStream_t st, float *out) {
    if (d.A == 64) hipLaunchKernelGGL(k_pack_obs<64>, dim3(d.W, GD_PACK_PARTS), dim3(256), 0, st, d, out);
    else hipLaunchKernelGGL(k_pack_obs<128>, dim3(d.W, GD_PACK_PARTS), dim3(256), 0, st, d, out);
}

void launch_pack_obs_rows(const DevSim &d, hipStream_t st, float *out, const float *weights) {
    if (d.n_rows == 0) return;
    if (weights) {  // the conditioned rows
        DevSim dc = d;
        dc.pack_weights = weights;
        if (d.A == 64) hipLaunchKernelGGL((k_pack_obs<64, true, true>), dim3(d.n_rows), dim3(256), 0, st, dc, out);
        else hipLaunchKernelGGL((k_pack_obs<128, true, true>), dim3(d.n_rows), dim3(256), 0, st, dc, out);
        return;
    }
    if (d.A == 64) hipLaunchKernelGGL((k_pack_obs<64, true>), dim3(d.n_rows), dim3(256), 0, st, d, out);
    else hipLaunchKernelGGL((k_pack_obs<128, true>), dim3(d.n_rows), dim3(256), 0, st, d, out);
}

void launch_pack_obs_conditioned(const DevSim &d, hipStream_t st, const float *weights, float *out) {
    if (d.pack && !d.pack_rows) {  // the attached buffer is current (its raw rows may not be)
        const size_t D = 6 + (size_t)(d.A - 1) * 6 + K * 13, groups = (size_t)d.W * d.A * (D + 3) / 4;
        const dim3 grid((unsigned)((groups + 255) / 256));
        if (d.A == 64) hipLaunchKernelGGL(k_pack_relayout<64>, grid, dim3(256), 0, st, d.pack, weights, out, groups);
        else hipLaunchKernelGGL(k_pack_relayout<128>, grid, dim3(256), 0, st, d.pack, weights, out, groups);
        return;
    }
    if (d.A == 64) hipLaunchKernelGGL(k_pack_obs_cond<64>, dim3(d.W, GD_PACK_PARTS), dim3(256), 0, st, d, weights, out);
    else hipLaunchKernelGGL(k_pack_obs_cond<128>, dim3(d.W, GD_PACK_PARTS), dim3(256), 0, st, d, weights, out);
}

void launch_expert_actions(const DevSim &d, hipStream_t st, float *actions, float *pos, float *vel, float *yaw, int *valid) {
    const size_t n = (size_t)d.W * d.A * GD_EPISODE_LEN;
    hipLaunchKernelGGL(k_expert_actions, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d, actions, pos, vel, yaw, valid);
}

void launch_set_log_actions(const DevSim &d, hipStream_t st, int t) {
    hipLaunchKernelGGL(k_set_log_actions, dim3((d.W * d.A + 255) / 256), dim3(256), 0, st, d, t);
}

}  // namespace gd
