"""The reference's closed-loop script, restated: `run()` of baselines/il/test/simulation.py:22-135, the yardstick of the
closed-loop BC driver (gd_bc_rollout, gpudrive_lab_amd.bc_rollout).  Test infrastructure for test_bc_rollout.py and
test_gpu_bc_rollout.py; it never imports the driver.

  metrics(done, info, xy)   simulation.py:29-30, 45-47, 56-67, 99-108 in numpy on scripted per-step sequences
  summary(...)              simulation.py:113-114, 131-136 in float32
  closed_loop(h, policy)    the whole loop on the call-sequence harness with a `DeviceBCPolicy` called once per step on
                            obs[~dead]
  run_rule_host(...)        the driver of the host program of csrc/bc_rollout_rule.hpp (tests/bc_rollout_rule_host.cpp)

Differences from the reference, all outside the arithmetic:
  - `mask` stands where `env.cont_agent_mask` does; `num_stack` is the harness's, not the literal 5;
  - goal_step is the raw step index: the reference divides it by the expert's `done_step` from a CSV (simulation.py:66);
  - the goal distance is sqrt(x * x + y * y) in float32, one rounding per operation, where the reference calls
    torch.linalg.norm on the two columns;
  - torch's `.mean()` / `.sum()` have no stated order.  The flag sums are exact in any order; the progress sum is taken in the
    order csrc/bc_rollout_rule.hpp states: 256 lanes, lane l adds rows l, l + 256, ... ascending, then the lanes ascending;
  - the per-label grouping, the CSV and the videos are left out; nothing is printed;
  - one hook, `source`, for where the single-frame observation comes from (`sim.packed_observations`: the kernels' own bits).
    The loop then stacks the frames as env_torch.py:1209-1216 does and calls `h.make_partner_mask` itself;
  - the loop also returns what the policy saw last (window, masks) and per-step records (the actions written into the
    simulator, the dead flags before each step, the global pose of live rows), which the reference does not keep."""
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LANES = 256
f32 = np.float32
SUMMARY_NAMES = ("off_road_rate", "veh_coll_rate", "goal_rate", "collision_rate", "goal_progress", "goal_count", "n_rows",
                 "iterations")


def goal_distance(xy):
    """[..., 2] float32 -> sqrt(x * x + y * y), float32, one rounding per operation."""
    x, y = np.asarray(xy[..., 0], f32), np.asarray(xy[..., 1], f32)
    return np.sqrt((x * x).astype(f32) + (y * y).astype(f32)).astype(f32)


def ordered_sum(v):
    """The fixed summation order of csrc/bc_rollout_rule.hpp, float32."""
    v = np.asarray(v, f32)
    lanes = np.zeros(LANES, f32)
    for l in range(min(LANES, len(v))):
        s = f32(0)
        for x in v[l::LANES]:
            s = f32(s + x)
        lanes[l] = s
    total = f32(0)
    for s in lanes:
        total = f32(total + s)
    return total


def summary(goal_achieved, off_road, veh_collision, init_goal_dist, goal_dist, iterations):
    """simulation.py:113-114, 131-136: the eight numbers, float32."""
    goal, off, veh = (np.asarray(a, f32) for a in (goal_achieved, off_road, veh_collision))
    n = f32(len(goal))
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = (np.asarray(goal_dist, f32) / np.asarray(init_goal_dist, f32)).astype(f32)  # (not guarded, as in the reference)
        ratio[goal.astype(bool)] = 0
        progress = (f32(1) - ratio).astype(f32)
        sums = [ordered_sum(a) for a in (off, veh, goal, progress)]
        off_rate, veh_rate, goal_rate = f32(sums[0] / n), f32(sums[1] / n), f32(sums[2] / n)
        return np.array([off_rate, veh_rate, goal_rate, f32(off_rate + veh_rate), f32(sums[3] / n), sums[2], n, f32(iterations)], f32)


def metrics(done, info, xy):
    """done [T + 1][N] int, info [T + 1][N][5] int, xy [T + 1][N][2] float32: state 0 is the reset state, state t + 1 what is read
    after step t.  Returns the per-row outputs, the iterations run and the summary."""
    done, info, xy = np.asarray(done), np.asarray(info), np.asarray(xy, f32)
    T, N = done.shape[0] - 1, done.shape[1]
    init_goal_dist = goal_distance(xy[0])                     # simulation.py:29-30
    dist_metrics = np.zeros(N, f32)
    infos = info[0]                                           # :32
    goal_ts, off_ts = np.full(N, -1, np.int32), np.full(N, -1, np.int32)
    off_road_ep = infos[:, 0].astype(np.int64).copy()         # :45-47
    veh_collision_ep = (infos[:, 1] + infos[:, 2]).astype(np.int64)
    goal_achieved_ep = infos[:, 3].astype(np.int64).copy()
    dead = np.zeros(N, bool)                                  # :25 (every row is a controlled agent)
    iterations = 0
    for t in range(T):
        iterations += 1
        dist_metrics[:] = goal_distance(xy[t])                # :56-58, every row
        goal_mask = (infos[:, 3] > 0) & (goal_ts == -1)       # :61-67
        off_mask = (infos[:, 0] > 0) & (off_ts == -1)
        goal_ts[goal_mask] = t
        off_ts[off_mask] = t
        dones, infos = done[t + 1], info[t + 1]               # :92-98
        off_road_ep = np.minimum(off_road_ep + infos[:, 0], 1)            # :99-104
        veh_collision_ep = np.minimum(veh_collision_ep + infos[:, 1] + infos[:, 2], 1)
        goal_achieved_ep = np.minimum(goal_achieved_ep + infos[:, 3], 1)
        dead = np.logical_or(dead, dones != 0)                # :105
        if dead.all():                                        # :107-108
            break
    out = dict(dead=dead, goal_achieved=goal_achieved_ep.astype(f32), off_road=off_road_ep.astype(f32),
               veh_collision=veh_collision_ep.astype(f32), goal_step=goal_ts, off_road_step=off_ts,
               init_goal_dist=init_goal_dist, goal_dist=dist_metrics, iterations=iterations)
    out["summary"] = summary(out["goal_achieved"], out["off_road"], out["veh_collision"], init_goal_dist, dist_metrics, iterations)
    return out


# ---- the host program of csrc/bc_rollout_rule.hpp
_HOST = {}


def rule_host(sanitize=False):
    """The compiled host program; sanitize: a second, stand-alone executable with -fsanitize=address,undefined."""
    if sanitize not in _HOST:
        out = os.path.join(tempfile.gettempdir(), "gd_bc_rollout_rule_host%s_%d" % ("_san" if sanitize else "", os.getuid()))
        src = os.path.join(HERE, "bc_rollout_rule_host.cpp")
        hdr = os.path.join(HERE, "..", "gpudrive_lab_amd", "csrc", "bc_rollout_rule.hpp")
        if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
            flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
            subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off"] + flags + ["-o", out, src])
        _HOST[sanitize] = out
    return _HOST[sanitize]


def run_rule_host(done, info, xy, sanitize=False):
    done, info, xy = np.asarray(done, np.int32), np.asarray(info, np.int32), np.asarray(xy, f32)
    T, N = done.shape[0] - 1, done.shape[1]
    assert info.shape == (T + 1, N, 5) and xy.shape == (T + 1, N, 2)
    with tempfile.TemporaryDirectory() as d:
        fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        with open(fin, "wb") as f:
            f.write(np.array([N, T], np.int32).tobytes() + done.tobytes() + info.tobytes() + xy.tobytes())
        subprocess.check_call([rule_host(sanitize), fin, fout])
        raw = open(fout, "rb").read()
    assert len(raw) == 4 * (8 * N + 92 + 8)
    i32, f = np.frombuffer(raw, np.int32), np.frombuffer(raw, f32)
    names = (("dead", i32), ("goal_achieved", f), ("off_road", f), ("veh_collision", f), ("goal_step", i32), ("off_road_step", i32),
             ("init_goal_dist", f), ("goal_dist", f))
    out = {k: a[j * N:(j + 1) * N].copy() for j, (k, a) in enumerate(names)}
    out["dead"] = out["dead"] != 0
    out["any_alive"] = i32[8 * N:8 * N + 92].copy()
    out["iterations"] = int(out["any_alive"][:91].sum())
    out["summary"] = f[8 * N + 92:].copy()
    return out


# ---- the whole loop on the harness
def closed_loop(h, policy, mask=None, n_steps=None, source=None, deterministic=True, u=None, z=None):
    """simulation.py:22-108 on `h`, a `TorchCallSequence(sim, dynamics_model=..., num_stack=R)`, with `policy`, a
    `DeviceBCPolicy`, called once per step on obs[~dead].  u [n_steps, N], z [n_steps, N, 3]: the draws of the rows
    (deterministic=False); a live row takes its own.  Returns a dict of device tensors and `iterations`."""
    import torch
    A, R, dev = h.max_agent_count, h.num_stack, h.device
    n_steps = h.episode_len if n_steps is None else n_steps
    state = {}

    def observe(reset=False):
        if source is None:
            o = h.reset() if reset else h.get_obs()
            return o, h.get_partner_mask()
        if reset:
            h.reset()
        frame = source().clone()
        pmask = h.make_partner_mask(frame[..., 6:6 + (A - 1) * 6]).clone()
        if R > 1:  # env_torch.py:1209-1216
            prev = torch.zeros_like(frame).repeat(1, 1, R - 1) if reset else state["stacked"][..., frame.shape[-1]:]
            state["stacked"] = torch.cat([prev, frame], dim=-1)
            frame = state["stacked"].clone()
        return frame, pmask

    def norm(p):
        x, y = p[:, 0], p[:, 1]
        return torch.sqrt(x * x + y * y)

    obs, partner_mask = observe(reset=True)                                   # simulation.py:23
    cont = (h.cont_agent_mask if mask is None else mask).to(dev)
    alive_agent_mask = cont.clone()                                           # :24
    dead_agent_mask = ~cont.clone()                                           # :25
    N = int(cont.sum())
    D = obs.shape[-1] // R                                                    # :28
    lo = D * (R - 1) + 3
    init_goal_dist = norm(obs[alive_agent_mask][:, lo:lo + 2])                # :29-30
    dist_metrics = torch.zeros_like(alive_agent_mask, dtype=torch.float32)    # :31
    infos = h.get_infos()                                                     # :32
    goal_timesteps = torch.full((N,), -1, dtype=torch.int32, device=dev)      # :33 (raw step indices)
    off_road_timesteps = torch.full((N,), -1, dtype=torch.int32, device=dev)  # :34
    off_road_ep = infos.off_road[alive_agent_mask].clone()                    # :45-47
    veh_collision_ep = infos.collided[alive_agent_mask].clone()
    goal_achieved_ep = infos.goal_achieved[alive_agent_mask].clone()
    T = h.episode_len
    rec = dict(actions=torch.zeros((N, T, 3), device=dev), dead_mask=torch.ones((N, T), dtype=torch.bool, device=dev),
               ego_global_pos=torch.zeros((N, T, 2), device=dev), ego_global_rot=torch.zeros((N, T), device=dev))
    last = {}
    iterations = 0
    for time_step in range(n_steps):
        iterations += 1
        all_actions = torch.zeros(obs.shape[0], obs.shape[1], 3, device=dev)  # :50
        road_mask = h.get_road_mask().to(dev)                                 # :53
        partner_mask_bool = partner_mask == 2                                 # :55
        dist_metrics[alive_agent_mask] = norm(obs[alive_agent_mask][:, lo:lo + 2])  # :56-58
        off_road = infos.off_road[alive_agent_mask]                           # :61-67
        goal_achieved = infos.goal_achieved[alive_agent_mask]
        goal_mask = (goal_achieved > 0) & (goal_timesteps == -1)
        off_road_mask = (off_road > 0) & (off_road_timesteps == -1)
        goal_timesteps[goal_mask] = time_step
        off_road_timesteps[off_road_mask] = time_step

        live = ~dead_agent_mask                                               # :69-76
        alive_obs = obs[live].view(-1, R, D).contiguous()
        B = alive_obs.shape[0]
        pm = torch.zeros((B, R, A - 1), dtype=torch.bool, device=dev)
        rm = torch.zeros((B, R, 200), dtype=torch.bool, device=dev)
        pm[:, R - 1], rm[:, R - 1] = partner_mask_bool[live], road_mask[live]
        rows = live[alive_agent_mask]  # which of the N rows are in the batch
        if deterministic:
            actions = policy(alive_obs, pm, rm, deterministic=True)
        else:
            actions = policy(alive_obs, pm, rm, u=u[time_step][rows].contiguous(), z=z[time_step][rows].contiguous())
        all_actions[live, :] = actions.squeeze(1)

        rec["actions"][:, time_step] = all_actions[alive_agent_mask]
        rec["dead_mask"][:, time_step] = dead_agent_mask[alive_agent_mask]
        pose = h.sim.absolute_self_observation_tensor().to_torch().to(dev)[alive_agent_mask]
        rec["ego_global_pos"][rows, time_step] = pose[rows][:, 0:2]
        rec["ego_global_rot"][rows, time_step] = pose[rows][:, 7]
        last = dict(window=obs[alive_agent_mask].view(N, R, D).clone(), partner_value=partner_mask[alive_agent_mask].clone(),
                    partner_mask=partner_mask_bool[alive_agent_mask].clone(), road_mask=road_mask[alive_agent_mask].clone())

        h.step_dynamics(all_actions)                                          # :92
        obs, partner_mask = observe()                                         # :96
        dones = h.get_dones()                                                 # :97
        infos = h.get_infos()                                                 # :98
        off_road_ep += infos.off_road[alive_agent_mask]                       # :99-104
        veh_collision_ep += infos.collided[alive_agent_mask]
        goal_achieved_ep += infos.goal_achieved[alive_agent_mask]
        off_road_ep = torch.clamp(off_road_ep, max=1)
        veh_collision_ep = torch.clamp(veh_collision_ep, max=1)
        goal_achieved_ep = torch.clamp(goal_achieved_ep, max=1)
        dead_agent_mask = torch.logical_or(dead_agent_mask, dones.to(dev))    # :105
        if (dead_agent_mask == True).all():  # noqa: E712 (the reference's spelling)  :107-108
            break
    out = dict(goal_achieved=goal_achieved_ep.to(torch.float32), off_road=off_road_ep.to(torch.float32),
               veh_collision=veh_collision_ep.to(torch.float32), goal_step=goal_timesteps, off_road_step=off_road_timesteps,
               init_goal_dist=init_goal_dist, goal_dist=dist_metrics[alive_agent_mask], dead=dead_agent_mask[alive_agent_mask],
               iterations=iterations, all_actions=all_actions)
    out.update(rec)
    out.update(last)
    host = lambda k: out[k].cpu().numpy()
    out["summary"] = summary(host("goal_achieved"), host("off_road"), host("veh_collision"), host("init_goal_dist"),
                             host("goal_dist"), iterations)
    return out
