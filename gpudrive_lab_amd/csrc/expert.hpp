// The logged (expert) action of one agent slot at one time step, as GPUDriveTorchEnv.get_expert_actions() hands it to the
// simulator (reference gpudrive/env/env_torch.py:1445-1509): the expert trajectory row ([pos 182 | vel 182 | yaw 91 |
// valid 91 | inferred action 910], gpudrive/datatypes/trajectory.py:24-41) sliced and clamped per dynamics model:
//   classic / bicycle : columns 0..2, accel in [-6, 6], steer in [-0.3, 0.3]
//   delta_local       : columns 0..2, dx, dy in [-6, 6], dyaw in [-pi, pi]
//   state             : (x, y, 1, yaw, vx, vy, 0, 0, 0, 0)
// torch.clamp = min(max(x, lo), hi) with NaN propagated.  Shared by the expert-action export and log playback (pack_obs.hip)
// and the warm-up of the device auto-reset (kernels.hip), so that both feed the same bits.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/gpudrive_amd.h"

namespace gd {

constexpr float kExpertPiF = 3.14159265358979323846f;  // torch.pi rounded to fp32

__device__ __forceinline__ float expert_clampf(float x, float lo, float hi) { return x != x ? x : fminf(fmaxf(x, lo), hi); }

// columns of the action the caller would feed for time step t of agent row `tr` (1456 floats): 10 for the State model, else 3
__device__ __forceinline__ void expert_action(const float *tr, int t, int model, float *act /*3 or 10*/) {
    constexpr int T = GD_EPISODE_LEN;
    const float *inf = tr + 6 * T + t * 10;
    if (model == GD_DYNAMICS_STATE) {
        act[0] = tr[2 * t]; act[1] = tr[2 * t + 1]; act[2] = 1.f; act[3] = tr[4 * T + t];
        act[4] = tr[2 * T + 2 * t]; act[5] = tr[2 * T + 2 * t + 1];
        act[6] = 0.f; act[7] = 0.f; act[8] = 0.f; act[9] = 0.f;
    } else if (model == GD_DYNAMICS_DELTA_LOCAL) {
        act[0] = expert_clampf(inf[0], -6.f, 6.f); act[1] = expert_clampf(inf[1], -6.f, 6.f);
        act[2] = expert_clampf(inf[2], -kExpertPiF, kExpertPiF);
    } else {
        act[0] = expert_clampf(inf[0], -6.f, 6.f); act[1] = expert_clampf(inf[1], -0.3f, 0.3f); act[2] = inf[2];
    }
}

}  // namespace gd
