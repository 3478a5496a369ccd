"""Episode bookkeeping on the device.

`EpisodeTracker` keeps what `PufferGPUDrive.step()` keeps (reference gpudrive/env/env_puffer.py:250-403):
live-agent mask, per-agent episode returns and lengths, collision / off-road counts, detection of
finished worlds, their statistics and their asynchronous reset -- in ONE kernel per step plus the
device-side reset pass, with no `.item()` / `.cpu()` synchronisation.  Field names follow the reference.

Reward types (gpudrive/env/env_torch.py:469-603): "weighted_combination", "sparse_on_goal_achieved", "reward_conditioned"
(every agent slot has its own three weights, `reward_weights_tensor` [W, A, 3], drawn per world at construction and again
for every world the tracker resets) and "distance_to_logs" (the weighted combination plus
`log_distance_weight * exp(-distance to the logged position)`, the logged position taken at the episode's step count).
Condition modes of the weights (env_torch.py:247-401): "random" draws `lb + u * (ub - lb)` per component, u from a
counter-based generator of (seed, world, draw, slot, component) -- it matches the reference (torch.rand) in distribution,
not value for value; "preset" and "fixed" match it in value."""
import ctypes as C

import numpy as np
import torch

from . import _capi

REWARD_TYPES = {"weighted_combination": _capi.EPISODE_REWARD_WEIGHTED, "sparse_on_goal_achieved": _capi.EPISODE_REWARD_SPARSE,
                "reward_conditioned": _capi.EPISODE_REWARD_CONDITIONED, "distance_to_logs": _capi.EPISODE_REWARD_LOG_DISTANCE}
CONDITION_MODES = {"random": _capi.CONDITION_RANDOM, "preset": _capi.CONDITION_PRESET, "fixed": _capi.CONDITION_FIXED}
WARMUP_SCOPES = {"reset_worlds": _capi.WARMUP_RESET_WORLDS, "all_worlds": _capi.WARMUP_ALL_WORLDS}


def check_warmup(init_steps, warmup):
    """(init_steps, scope code) for the warm-up of the device auto-reset; ValueError for init_steps outside [0, 90] (or not
    an integer) and for an unknown scope.  Host only."""
    if isinstance(init_steps, bool) or not isinstance(init_steps, (int, np.integer)):
        raise ValueError("init_steps must be an integer in [0, %d], got %r" % (_capi.INIT_STEPS_MAX, init_steps))
    if not 0 <= int(init_steps) <= _capi.INIT_STEPS_MAX:
        raise ValueError("init_steps must be in [0, %d] (the expert trajectory has 91 steps), got %d"
                         % (_capi.INIT_STEPS_MAX, init_steps))
    if warmup not in WARMUP_SCOPES:
        raise ValueError("unknown warmup scope %r (one of %s)" % (warmup, sorted(WARMUP_SCOPES)))
    return int(init_steps), WARMUP_SCOPES[warmup]
# bounds of (collision, goal_achieved, off_road), gpudrive/env/config.py:103-113
DEFAULT_LB = (-1.0, 1.0, -1.0)
DEFAULT_UB = (0.0, 2.0, 0.0)
# the named weight sets, from the bounds (env_torch.py:290-345), in Python floats
PRESETS = {
    "cautious": lambda lb, ub: (lb[0] * 0.9, ub[1] * 0.7, lb[2] * 0.9),
    "aggressive": lambda lb, ub: (lb[0] * 0.5, ub[1] * 0.9, lb[2] * 0.6),
    "balanced": lambda lb, ub: ((lb[0] + ub[0]) / 2, (lb[1] + ub[1]) / 2, (lb[2] + ub[2]) / 2),
    "risk_taker": lambda lb, ub: (lb[0] * 0.3, ub[1], lb[2] * 0.4),
}


def resolve_condition(condition_mode, agent_type=None, lb=DEFAULT_LB, ub=DEFAULT_UB):
    """(mode code, float32[3] weights) for a condition mode; the weights are zero for "random".  Host only: raises
    ValueError for an unknown mode or preset name and for a "fixed" `agent_type` whose shape is not (3,)."""
    if condition_mode not in CONDITION_MODES:
        raise ValueError("unknown condition_mode %r (one of %s)" % (condition_mode, sorted(CONDITION_MODES)))
    if condition_mode == "random":
        return CONDITION_MODES["random"], np.zeros(3, np.float32)
    if condition_mode == "preset":
        if not isinstance(agent_type, str) or agent_type not in PRESETS:
            raise ValueError("unknown agent_type %r for condition_mode='preset' (one of %s)" % (agent_type, sorted(PRESETS)))
        lb, ub = [float(x) for x in lb], [float(x) for x in ub]
        return CONDITION_MODES["preset"], np.asarray(PRESETS[agent_type](lb, ub), np.float32)
    if agent_type is None or isinstance(agent_type, str):
        raise ValueError("condition_mode='fixed' needs agent_type: a tensor of shape [3]")
    w = agent_type.detach().cpu().numpy() if isinstance(agent_type, torch.Tensor) else np.asarray(agent_type)
    if w.shape != (3,):
        raise ValueError("agent_type must have shape [3], got %s" % (tuple(w.shape),))
    return CONDITION_MODES["fixed"], w.astype(np.float32)


class EpisodeTracker:
    def __init__(self, sim, collision_weight=-0.5, goal_achieved_weight=1.0, off_road_weight=-0.5,
                 reward_type="weighted_combination", auto_reset=True, *, condition_mode="random", agent_type=None,
                 reward_weight_lb=DEFAULT_LB, reward_weight_ub=DEFAULT_UB, log_distance_weight=0.01, seed=0,
                 init_steps=0, warmup="reset_worlds"):
        """reward_type: a key of REWARD_TYPES.  reward_conditioned: `condition_mode` / `agent_type` say how the weights of
        every world are drawn, now and whenever the tracker resets a world (see `set_reward_weights`); `reward_weight_lb`
        / `_ub` are the (collision, goal_achieved, off_road) bounds of "random" and of the presets; `seed` keys "random".
        distance_to_logs: `log_distance_weight` scales the distance term.
        init_steps: the reference's warm-up (`init_steps`, 0..90): every world the tracker resets is then advanced that many
        steps with the logged actions, on the device, before its observations are written.  warmup: "reset_worlds" (only
        the worlds reset in this step) or "all_worlds" (the reference as it is: every world, whenever any world is reset).
        The episode bookkeeping is unchanged.  The setting belongs to the simulator: a tracker built later replaces it."""
        self.init_steps, warm_scope = check_warmup(init_steps, warmup)
        self.warmup = warmup
        if reward_type not in REWARD_TYPES:
            raise ValueError("unknown reward_type %r (one of %s)" % (reward_type, sorted(REWARD_TYPES)))
        self.sim = sim
        self._L = _capi.lib()
        W, A = sim._W, sim._A
        dev = sim.controlled_state_tensor().to_torch().device
        # cont_agent_mask, captured once like gpudrive/env/env_torch.py:61-63 does at construction
        self.controlled_agent_mask = sim.controlled_state_tensor().to_torch().clone().squeeze(-1) == 1
        self.num_agents = None  # filled lazily: a device->host sync the step path never needs
        self.cfg = _capi.GdEpisodeConfig(float(collision_weight), float(goal_achieved_weight), float(off_road_weight),
                                         REWARD_TYPES[reward_type], 1 if auto_reset else 0)
        z = lambda dt: torch.zeros((W, A), dtype=dt, device=dev)
        self.agent_episode_returns, self.episode_lengths = z(torch.float32), z(torch.float32)
        self.collided_in_episode, self.offroad_in_episode = z(torch.float32), z(torch.float32)
        self.live_agent_mask = torch.ones((W, A), dtype=torch.bool, device=dev)  # env_puffer.py:221-223
        self.rewards, self.terminals = z(torch.float32), z(torch.bool)
        self.truncations, self.masks = z(torch.bool), z(torch.bool)
        self.done_worlds = torch.zeros((W,), dtype=torch.int32, device=dev)
        self.stats = torch.zeros((_capi.EPISODE_STATS,), dtype=torch.float32, device=dev)
        self.world_stats = torch.zeros((W, _capi.EPISODE_STATS), dtype=torch.float32, device=dev)
        self._cmask_u8 = self.controlled_agent_mask.to(torch.uint8).contiguous()
        p = lambda t: C.c_void_p(t.data_ptr())
        self._bufs = _capi.GdEpisodeBuffersRows(
            p(self._cmask_u8), p(self.agent_episode_returns), p(self.episode_lengths), p(self.collided_in_episode),
            p(self.offroad_in_episode), p(self.live_agent_mask), p(self.rewards), p(self.terminals), p(self.truncations),
            p(self.masks), p(self.done_worlds), p(self.stats), p(self.world_stats))
        self._lb = tuple(float(x) for x in reward_weight_lb)
        self._ub = tuple(float(x) for x in reward_weight_ub)
        if len(self._lb) != 3 or len(self._ub) != 3:
            raise ValueError("reward_weight_lb / reward_weight_ub need three components (collision, goal_achieved, off_road)")
        self.reward_weights_tensor = None  # [W, A, 3] f32: reward_conditioned only (or after set_reward_weights)
        self.weight_draws = None           # [W] int32: draws of each world's weights so far
        if reward_type == "distance_to_logs":
            self.cfg.log_distance_weight = float(log_distance_weight)
        self.cfg.seed = int(seed) & (2 ** 64 - 1)
        for j in range(3):
            self.cfg.lb[j], self.cfg.ub[j] = self._lb[j], self._ub[j]
        if reward_type == "reward_conditioned":
            self._set_condition(self.cfg, condition_mode, agent_type)
            self.set_reward_weights(condition_mode=condition_mode, agent_type=agent_type)  # draw 0 of every world
        _capi.check(self._L.gd_episode_set_warmup(sim._h, self.init_steps, warm_scope), "gd_episode_set_warmup")

    def _set_condition(self, cfg, condition_mode, agent_type):
        mode, w = resolve_condition(condition_mode, agent_type, self._lb, self._ub)
        cfg.condition_mode = mode
        for j in range(3):
            cfg.weights[j] = float(w[j])

    def set_reward_weights(self, worlds=None, condition_mode="random", agent_type=None):
        """Draw new reward weights for the listed worlds (None: all) into `reward_weights_tensor`, on the device
        (the reference's _set_reward_weights(env_idx_list, condition_mode, agent_type), env_torch.py:247-401).
        "random": a new draw of the generator (see the module docstring); "preset": agent_type names one of PRESETS;
        "fixed": agent_type is a tensor of shape [3].  Arguments are checked before anything reaches the device
        (ValueError).  The mode the tracker redraws reset worlds in is the one given at construction."""
        cfg = _capi.GdEpisodeConfig.from_buffer_copy(self.cfg)
        self._set_condition(cfg, condition_mode, agent_type)
        idx = None
        if worlds is not None:
            if hasattr(worlds, "detach"):
                worlds = worlds.detach().cpu().numpy()
            idx = np.ascontiguousarray(np.atleast_1d(np.asarray(worlds)).astype(np.int32).ravel())
            if ((idx < 0) | (idx >= self.sim._W)).any():
                raise ValueError("set_reward_weights: world index out of range")
        if self.reward_weights_tensor is None:
            W, A = self.sim._W, self.sim._A
            dev = self.rewards.device
            self.reward_weights_tensor = torch.zeros((W, A, 3), dtype=torch.float32, device=dev)
            self.weight_draws = torch.zeros((W,), dtype=torch.int32, device=dev)
            self._bufs.reward_weights = self.reward_weights_tensor.data_ptr()
            self._bufs.weight_draws = self.weight_draws.data_ptr()
        self.sim._bind_stream()
        if idx is None:
            rc = self._L.gd_episode_draw_weights(self.sim._h, C.byref(cfg), C.byref(self._bufs), None, 0)
        else:
            rc = self._L.gd_episode_draw_weights(self.sim._h, C.byref(cfg), C.byref(self._bufs),
                                                 idx.ctypes.data_as(C.POINTER(C.c_int32)), len(idx))
        _capi.check(rc, "gd_episode_draw_weights")
        return self.reward_weights_tensor

    def step(self, step_sim=True):
        """sim.step() (actions are already in the action tensor), then the bookkeeping kernel and the
        device-side reset of the worlds that just finished.  Returns full [W, A] tensors
        (rewards, terminals, truncations, masks); index them with `controlled_agent_mask` to get the
        flat per-agent views PufferGPUDrive returns.  Nothing here waits for the device."""
        if step_sim:
            self.sim.step()
        self.sim._bind_stream()
        _capi.check(self._L.gd_episode_step(self.sim._h, C.byref(self.cfg), C.byref(self._bufs)), "gd_episode_step")
        return self.rewards, self.terminals, self.truncations, self.masks

    def pop_stats(self):
        """Running sums over the episodes finished since the last call, as the dictionary PufferGPUDrive
        logs (env_puffer.py:352-371); the one place that synchronises with the device."""
        s = self.stats.cpu().tolist()
        self.stats.zero_()
        if self.num_agents is None:
            self.num_agents = int(self.controlled_agent_mask.sum().item())
        ep, fin = s[0], s[1]
        if ep == 0 or fin == 0:
            return {}
        A = self.controlled_agent_mask.shape[1]
        return {
            "mean_episode_reward_per_agent": s[2] / fin,
            "perc_goal_achieved": s[5] / fin,
            "perc_off_road": s[3] / fin,
            "perc_veh_collisions": s[4] / fin,
            "total_controlled_agents": self.num_agents,
            "control_density": self.num_agents / self.controlled_agent_mask.numel(),
            "episode_length": s[7] / (ep * A),
            "perc_truncated": s[6] / fin,
            "num_completed_episodes": int(ep),
            "total_collisions": s[8],
            "total_off_road": s[9],
        }
