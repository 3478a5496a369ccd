"""The reference's evaluation rollout (examples/experimental/eval_utils.py rollout(), lines 94-227), restated for the tests of the
closed-loop PPO evaluator (gd_policy_rollout, gpudrive_lab_amd.ppo_rollout).  Test infrastructure for test_ppo_rollout.py and
test_gpu_ppo_rollout.py; it never imports the evaluator.

  metrics(mask, done, info)   the bookkeeping in numpy on scripted (done, info) sequences: the rule
  run_rule_host(...)          the driver of the host program of csrc/policy_rollout_rule.hpp (tests/policy_rollout_rule_host.cpp)
  closed_loop(sim, policy...) the whole loop in torch over a simulator and a `DevicePolicy`, called on the compacted rows

Both restatements keep [W, A] arrays and the reference's order of operations: the sums of the rows live before the step, then
live[dones] = False, then the world test on the done flags as they are now, then the `break`."""
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
f32 = np.float32
T_MAX = 91
SUMMARY_NAMES = ("goal_achieved", "collided", "off_road", "other", "n_rows", "worlds_with_rows", "iterations",
                 "mean_episode_length")
WORLD_NAMES = ("goal_achieved_count", "frac_goal_achieved", "collided_count", "frac_collided", "off_road_count", "frac_off_road",
               "other_count", "frac_other", "controlled_per_scene")


def ordered_sum(v):
    """The fixed summation order of csrc/policy_rollout_rule.hpp, float32: 256 lanes, lane l adds entries l, l + 256, ...
    ascending, then the lanes ascending."""
    v = np.asarray(v, f32)
    lanes = np.zeros(256, f32)
    for i in range(0, len(v), 256):
        chunk = v[i:i + 256]
        lanes[:len(chunk)] = lanes[:len(chunk)] + chunk
    total = f32(0)
    for s in lanes:
        total = f32(total + s)
    return total


def counts(mask, goal, collided, off_road):
    """eval_utils.py:190-212 in numpy float32: the per-world counts and fractions."""
    controlled = mask.sum(1).astype(f32)
    out = {"controlled_per_scene": controlled}
    out["goal_achieved_count"] = (goal > 0).astype(f32).sum(1, dtype=f32)
    out["collided_count"] = (collided > 0).astype(f32).sum(1, dtype=f32)
    out["off_road_count"] = (off_road > 0).astype(f32).sum(1, dtype=f32)
    out["other_count"] = ((goal == 0) & ((collided == 0) & ((off_road == 0) & mask))).astype(f32).sum(1, dtype=f32)
    with np.errstate(invalid="ignore", divide="ignore"):
        for k in ("goal_achieved", "collided", "off_road", "other"):
            out["frac_" + k] = (out[k + "_count"] / controlled).astype(f32)
    return out


def summary(world, episode_lengths, any_active, n_steps):
    W = len(episode_lengths)
    return np.array([ordered_sum(world["goal_achieved_count"]), ordered_sum(world["collided_count"]),
                     ordered_sum(world["off_road_count"]), ordered_sum(world["other_count"]),
                     ordered_sum(world["controlled_per_scene"]), ordered_sum((world["controlled_per_scene"] > 0).astype(f32)),
                     f32(int(any_active[:n_steps].sum())), f32(ordered_sum(episode_lengths) / f32(W))], f32)


def metrics(mask, done, info):
    """mask [W, A] bool; done [T, W, A] and info [T, W, A, 5] int32, entry t what is read AFTER step t.  Returns the per-slot
    sums and live flags ([W, A]), the per-world results, any_active [92], iterations and the summary."""
    mask = np.asarray(mask, bool)
    done, info = np.asarray(done, np.int32), np.asarray(info, np.int32)
    T, (W, A) = done.shape[0], mask.shape
    goal, collided, off_road = (np.zeros((W, A), f32) for _ in range(3))   # eval_utils.py:105-107
    active_worlds = list(range(W))                                          # :108
    episode_lengths = np.zeros(W, f32)                                      # :109
    live = mask.copy()                                                      # :112
    any_active = np.zeros(T_MAX + 1, np.int32)
    any_active[0] = 1
    iterations = 0
    for t in range(T):                                                      # :114
        iterations += 1
        dones = done[t] != 0                                                # :159
        off_road[live] += info[t][..., 0][live].astype(f32)                 # :162-164
        collided[live] += (info[t][..., 1] + info[t][..., 2])[live].astype(f32)
        goal[live] += info[t][..., 3][live].astype(f32)
        live[dones] = False                                                 # :167
        n_done = (dones & mask).sum(1)                                      # :170-174
        total = mask.sum(1)
        for w in np.nonzero(n_done == total)[0]:                            # :176-179
            if w in active_worlds:
                active_worlds.remove(w)
                episode_lengths[w] = t
        if not active_worlds:                                               # :187-188
            break
        any_active[t + 1] = 1
    out = dict(goal_achieved=goal, collided=collided, off_road=off_road, live=live, episode_lengths=episode_lengths,
               world_active=np.isin(np.arange(W), active_worlds), any_active=any_active, iterations=iterations)
    out.update(counts(mask, goal, collided, off_road))
    out["summary"] = summary(out, episode_lengths, any_active, T)
    return out


# ---- the host program of csrc/policy_rollout_rule.hpp
_HOST = {}


def rule_host(sanitize=False):
    """The compiled host program; sanitize: a second, stand-alone executable with -fsanitize=address,undefined."""
    if sanitize not in _HOST:
        out = os.path.join(tempfile.gettempdir(), "gd_policy_rollout_rule_host%s_%d" % ("_san" if sanitize else "", os.getuid()))
        src = os.path.join(HERE, "policy_rollout_rule_host.cpp")
        hdr = os.path.join(HERE, "..", "gpudrive_lab_amd", "csrc", "policy_rollout_rule.hpp")
        if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
            flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
            subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off"] + flags + ["-o", out, src])
        _HOST[sanitize] = out
    return _HOST[sanitize]


def run_rule_host(mask, done, info, sanitize=False):
    mask = np.asarray(mask, bool)
    done, info = np.asarray(done, np.int32), np.asarray(info, np.int32)
    T, (W, A) = done.shape[0], mask.shape
    assert done.shape == (T, W, A) and info.shape == (T, W, A, 5)
    with tempfile.TemporaryDirectory() as d:
        fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        with open(fin, "wb") as f:
            f.write(np.array([W, A, T], np.int32).tobytes() + mask.astype(np.int32).tobytes() + done.tobytes() + info.tobytes())
        subprocess.check_call([rule_host(sanitize), fin, fout])
        raw = open(fout, "rb").read()
    S = W * A
    assert len(raw) == 4 * (4 * S + 11 * W + 92 + 8)
    i32, f = np.frombuffer(raw, np.int32), np.frombuffer(raw, f32)
    out = {"live": i32[:S].reshape(W, A) != 0}
    for j, k in enumerate(("goal_achieved", "collided", "off_road")):
        out[k] = f[(j + 1) * S:(j + 2) * S].reshape(W, A).copy()
    o = 4 * S
    out["world_active"] = i32[o:o + W] != 0
    out["episode_lengths"] = f[o + W:o + 2 * W].copy()
    for j, k in enumerate(WORLD_NAMES):
        out[k] = f[o + (2 + j) * W:o + (3 + j) * W].copy()
    o += 11 * W
    out["any_active"] = i32[o:o + 92].copy()
    out["iterations"] = int(out["any_active"][:T].sum())
    out["summary"] = f[o + 92:].copy()
    return out


# ---- the whole loop over a simulator
def closed_loop(sim, policy, table, mask=None, n_steps=T_MAX, deterministic=False, u=None, init_steps=0, reward_weights=None):
    """eval_utils.py:94-227 on `sim`, a SimManager, with `policy`, a `DevicePolicy` (no dropout rule), called once per step
    on next_obs[live], the compacted rows, as the reference calls its network.  table: the [n_actions, 3] device action
    table.  u [n_steps, N]: the draws of the rows (deterministic=False); a live row takes its own.  The observation is
    `packed_observations()[live]`, the kernels' own bits.  Returns a dict of device tensors, and `iterations`."""
    import torch
    W, A, dev = sim._W, sim._A, sim._device

    def get_obs():
        return sim.packed_observations(reward_weights=reward_weights).clone()

    sim.reset(list(range(W)))                                                      # eval_utils.py:102 (env.reset ...
    if init_steps > 0:
        sim.advance_log_playback(init_steps)                                       # ... advances the log playback)
    next_obs = get_obs()
    goal_achieved = torch.zeros((W, A), device=dev)                                # :105-107
    collided = torch.zeros((W, A), device=dev)
    off_road = torch.zeros((W, A), device=dev)
    active_worlds = list(range(W))                                                 # :108
    episode_lengths = torch.zeros(W)                                               # :109
    control_mask = (sim.controlled_state_tensor().to_torch().squeeze(-1) == 1) if mask is None else mask.to(dev)
    live_agent_mask = control_mask.clone()                                         # :111-112
    N = int(control_mask.sum())
    rec = dict(actions_idx=torch.full((N, T_MAX), -1, dtype=torch.int64, device=dev),
               live_mask=torch.zeros((N, T_MAX), dtype=torch.bool, device=dev),
               agent_positions=torch.zeros((W, A, T_MAX, 2), device=dev))
    any_active = torch.zeros(T_MAX + 1, dtype=torch.int32)
    any_active[0] = 1
    iterations = 0
    last_live = live_agent_mask.clone()
    for time_step in range(n_steps):                                               # :114
        iterations += 1
        rows = live_agent_mask[control_mask]  # which of the N rows are in the batch
        rec["live_mask"][:, time_step] = rows
        last_live = live_agent_mask.clone()
        if live_agent_mask.any():                                                  # :119
            obs = next_obs[live_agent_mask].contiguous()
            if deterministic:
                action = policy(obs, deterministic=True)[0]
            else:
                action = policy(obs, u[time_step][rows].contiguous())[0]
            action_template = torch.zeros((W, A), dtype=torch.int64, device=dev)   # :125-128
            action_template[live_agent_mask] = action
            rec["actions_idx"][:, time_step] = torch.where(rows, action_template[control_mask], -1)
            sim.action_tensor().to_torch()[:, :, :3] = table[action_template]      # :131 (_apply_actions decodes the indices)
            sim.step()
        next_obs = get_obs()                                                       # :158-160
        dones = sim.done_tensor().to_torch().reshape(W, A).bool()
        info = sim.info_tensor().to_torch().reshape(W, A, 5)
        off_road[live_agent_mask] += info[..., 0][live_agent_mask].float()         # :162-164
        collided[live_agent_mask] += (info[..., 1] + info[..., 2])[live_agent_mask].float()
        goal_achieved[live_agent_mask] += info[..., 3][live_agent_mask].float()
        live_agent_mask[dones] = False                                             # :167
        num_dones_per_world = (dones & control_mask).sum(dim=1)                    # :170-174
        total_controlled_agents = control_mask.sum(dim=1)
        done_worlds = (num_dones_per_world == total_controlled_agents).nonzero(as_tuple=True)[0]
        for world in done_worlds.tolist():                                         # :176-179
            if world in active_worlds:
                active_worlds.remove(world)
                episode_lengths[world] = time_step
        pos = sim.absolute_self_observation_tensor().to_torch()                    # :181-184
        rec["agent_positions"][:, :, time_step, 0] = pos[..., 0]
        rec["agent_positions"][:, :, time_step, 1] = pos[..., 1]
        if not active_worlds:                                                      # :187-188
            break
        any_active[time_step + 1] = 1
    controlled_per_scene = control_mask.sum(dim=1).float()                         # :191
    goal_achieved_count = (goal_achieved > 0).float().sum(axis=1)                  # :194-206
    collided_count = (collided > 0).float().sum(axis=1)
    off_road_count = (off_road > 0).float().sum(axis=1)
    other_count = torch.logical_and(goal_achieved == 0, torch.logical_and(collided == 0, torch.logical_and(
        off_road == 0, control_mask))).float().sum(dim=1)
    out = dict(goal_achieved_count=goal_achieved_count, frac_goal_achieved=goal_achieved_count / controlled_per_scene,  # :209-212
               collided_count=collided_count, frac_collided=collided_count / controlled_per_scene,
               off_road_count=off_road_count, frac_off_road=off_road_count / controlled_per_scene,
               other_count=other_count, frac_other=other_count / controlled_per_scene,
               controlled_per_scene=controlled_per_scene, episode_lengths=episode_lengths.to(dev),
               goal_achieved=goal_achieved[control_mask], collided=collided[control_mask], off_road=off_road[control_mask],
               live=live_agent_mask[control_mask], last_live=last_live, control_mask=control_mask,
               any_active=any_active.to(dev), iterations=iterations, **rec)
    world = {k: out[k].cpu().numpy() for k in WORLD_NAMES}
    out["summary"] = summary(world, episode_lengths.numpy(), any_active.numpy(), n_steps)
    return out
