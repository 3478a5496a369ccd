"""The learner's step on the device: discrete action indices in, flat per-agent tensors out.

`DeviceLearnerEnv` is the shape of the reference's PPO environment (gpudrive/env/env_puffer.py:235-403): `step()` takes one
discrete action index per controlled agent and returns `obs[controlled_agent_mask]` as [N, D] with the rewards, terminals,
truncations and masks of the same N rows.  Here nothing is gathered after the fact: the engine's learner rows
(`SimManager.set_learner_rows`) map every controlled slot to its row once, and then

  - the indices are decoded through the action table into the action tensor by one kernel (`set_discrete_actions`),
  - the kernels that produce the packed observation write each controlled agent's row straight into the [N, D] buffer
    (`direct_pack_rows`), and no packed row for any other slot,
  - the episode kernel writes the four flat outputs through the same map (`EpisodeTracker` with learner rows).

One step is therefore: indices in, flat tensors out, no host synchronisation and nothing sized by padding slots.  The rows are
fixed until `resample()`; the tensors returned are the same buffers every step (overwritten in place).

`ConditionedLearnerEnv` is the same loop for the reward-conditioned policy (reward_type "reward_conditioned"): its rows are
[N, D + 3] = ego 6 | the slot's 3 reward weights | partners | road points, written in place by the same kernels
(`direct_pack_rows(reward_weights=...)`); the weights the tracker redraws for the worlds it resets reach the rows on the
device."""
from itertools import product

import torch

from .episode import DEFAULT_LB, DEFAULT_UB, EpisodeTracker, check_warmup, resolve_condition
from .harness import default_action_values

_DYNAMICS_NAMES = {0: "classic", 1: "bicycle", 2: "delta_local", 3: "state"}


def action_table(dynamics_model):
    """The discrete action table of `dynamics_model` ("classic", "bicycle" or "delta_local"): a float32 [n, 3] tensor whose
    row k is action index k, in `itertools.product(first, second, third)` order (reference _set_discrete_action_space,
    gpudrive/env/env_torch.py:666-724): 7 x 13 x 1 = 91 rows for classic / bicycle, 20^3 = 8000 for delta_local.
    ValueError for "state", which has no discrete action space."""
    if dynamics_model == "state":
        raise ValueError("action_table: the state dynamics model has no discrete action space")
    a1, a2, a3 = default_action_values(dynamics_model)
    return torch.tensor([[v1.item(), v2.item(), v3.item()] for v1, v2, v3 in product(a1, a2, a3)], dtype=torch.float32)


_default_table = action_table  # (the constructor's argument of the same name shadows it)


def _check_table(who, table):
    """ValueError unless `table` is None (the default table) or a [n, 3] tensor with n >= 1.  Host only."""
    if table is None:
        return
    if not isinstance(table, torch.Tensor) or table.dim() != 2 or table.shape[1] != 3 or table.shape[0] < 1:
        raise ValueError("%s: action_table must be a [n, 3] tensor, got %s"
                         % (who, tuple(table.shape) if isinstance(table, torch.Tensor) else type(table)))


class DeviceLearnerEnv:
    def __init__(self, sim, action_table=None, only=True, init_steps=0, warmup="reset_worlds", **tracker_kwargs):
        """sim: a SimManager.  action_table: float32 [n, 3] (default: `action_table()` of the simulator's dynamics model).
        only: the raw partner / road rows are not written any more (nothing but the learner rows).  init_steps / warmup:
        the reference's warm-up (its PPO config sets init_steps 11): with init_steps > 0 construction and `resample()`
        reset every world and advance it that many steps with the logged actions (PufferGPUDrive.__init__ /
        resample_scenario_batch through env.reset), and the worlds `step()` resets are warmed on the device (see
        `EpisodeTracker`).  tracker_kwargs go to `EpisodeTracker` (reward weights, reward_type, auto_reset, ...);
        "reward_conditioned" is not supported here: its [N, D + 3] rows are `ConditionedLearnerEnv`'s.  Arguments are
        checked before anything reaches the device (ValueError)."""
        check_warmup(init_steps, warmup)
        if tracker_kwargs.get("reward_type") == "reward_conditioned":
            raise ValueError("DeviceLearnerEnv: reward_type='reward_conditioned' ([N, D + 3] rows) is not supported; "
                             "use ConditionedLearnerEnv")
        _check_table(type(self).__name__, action_table)
        self._init(sim, action_table, only, init_steps, warmup, tracker_kwargs)

    def _init(self, sim, action_table, only, init_steps, warmup, tracker_kwargs):
        """Everything after the argument checks: the first access to the simulator."""
        if action_table is None:
            action_table = _default_table(_DYNAMICS_NAMES[int(sim._params.dynamicsModel)])
        self.sim = sim
        self.only = bool(only)
        self.init_steps = int(init_steps)
        self._tracker_kwargs = dict(tracker_kwargs, init_steps=self.init_steps, warmup=warmup)
        self.table = action_table.to(device=sim._device, dtype=torch.float32).contiguous()
        if self.init_steps > 0:
            sim.reset(list(range(sim._W)))
        self._setup()
        self._warm_up()

    def _warm_up(self):
        """The host warm-up of construction and resample (env.reset -> advance_sim_with_log_playback).  It runs after the
        rows are attached: attaching runs a reset pass, whose collision re-run on the warmed state the reference does not
        have."""
        if self.init_steps > 0:
            self.sim.advance_log_playback(self.init_steps)

    def _setup(self):
        """Tracker (it captures the controlled mask), learner rows from that mask, the row buffer, the flat outputs."""
        sim = self.sim
        self.tracker = EpisodeTracker(sim, **self._tracker_kwargs)
        self.controlled_agent_mask = self.tracker.controlled_agent_mask
        n = sim.set_learner_rows(self.controlled_agent_mask)  # the one host synchronisation, at setup
        self.num_agents = n
        self.obs = self._attach()
        dev = self.table.device
        m = max(n, 1)  # (real allocations for n = 0)
        self.rewards = torch.zeros((m,), dtype=torch.float32, device=dev)[:n]
        self.terminals = torch.zeros((m,), dtype=torch.bool, device=dev)[:n]
        self.truncations = torch.zeros((m,), dtype=torch.bool, device=dev)[:n]
        self.masks = torch.zeros((m,), dtype=torch.bool, device=dev)[:n]
        b = self.tracker._bufs
        b.reward_rows, b.terminal_rows = self.rewards.data_ptr(), self.terminals.data_ptr()
        b.truncated_rows, b.mask_rows = self.truncations.data_ptr(), self.masks.data_ptr()

    def _attach(self):
        """Attach the row buffer the step's kernels write (after the learner rows are set); returns it."""
        return self.sim.direct_pack_rows(only=self.only)

    def reset(self):
        """Empty the episode storage (PufferGPUDrive.reset, env_puffer.py:200-233) and return the [N, D] observations of
        the current state."""
        t = self.tracker
        for x in (t.agent_episode_returns, t.episode_lengths, t.collided_in_episode, t.offroad_in_episode):
            x.zero_()
        t.live_agent_mask.fill_(True)
        return self.obs

    def step(self, actions):
        """actions: int64 [N] device tensor of action indices.  Decodes them into the action tensor, steps the simulator,
        runs the episode bookkeeping (finished worlds reset on the device) and returns
        (obs [N, D], rewards [N], terminals [N], truncations [N], masks [N]).  No host synchronisation."""
        self.sim.set_discrete_actions(actions, self.table)
        self.tracker.step()
        return self.obs, self.rewards, self.terminals, self.truncations, self.masks

    def pop_stats(self):
        return self.tracker.pop_stats()

    def resample(self, scenes):
        """A new batch of scenes (the reference's resample_scenario_batch, env_puffer.py:438-453): set_maps, the controlled
        mask derived again, the learner rows set from it, the row buffer attached again, the warm-up (init_steps), the
        storage emptied.  Returns the [N, D] observations of the new worlds."""
        self.sim.set_maps(scenes)
        self._setup()
        self._warm_up()
        return self.reset()


class ConditionedLearnerEnv(DeviceLearnerEnv):
    def __init__(self, sim, action_table=None, only=True, init_steps=0, warmup="reset_worlds", *, condition_mode="random",
                 agent_type=None, **tracker_kwargs):
        """`DeviceLearnerEnv` for the reward-conditioned policy (reward_type "reward_conditioned", gpudrive/networks/
        late_fusion.py:104-110): `obs` is [N, D + 3] = ego 6 | the slot's 3 reward weights | partners | road points
        (env_torch.py:756-810), `packed_observations(reward_weights=reward_weights_tensor)[mask]` bit for bit, written in
        place by the step's kernels.  condition_mode / agent_type: how the tracker draws every world's weights, at
        construction and for every world it resets ("random", "preset" with a preset name, "fixed" with a [3] tensor; see
        `EpisodeTracker`).  tracker_kwargs go to `EpisodeTracker`; a reward_type other than "reward_conditioned" is refused.
        Arguments are checked before anything reaches the device (ValueError)."""
        check_warmup(init_steps, warmup)
        rt = tracker_kwargs.pop("reward_type", "reward_conditioned")
        if rt != "reward_conditioned":
            raise ValueError("ConditionedLearnerEnv: reward_type must be 'reward_conditioned', got %r (DeviceLearnerEnv "
                             "takes the others)" % (rt,))
        lb = tracker_kwargs.get("reward_weight_lb", DEFAULT_LB)
        ub = tracker_kwargs.get("reward_weight_ub", DEFAULT_UB)
        if len(tuple(lb)) != 3 or len(tuple(ub)) != 3:
            raise ValueError("reward_weight_lb / reward_weight_ub need three components (collision, goal_achieved, off_road)")
        resolve_condition(condition_mode, agent_type, lb, ub)
        _check_table(type(self).__name__, action_table)
        self.condition_mode, self.agent_type = condition_mode, agent_type
        self._init(sim, action_table, only, init_steps, warmup,
                   dict(tracker_kwargs, reward_type="reward_conditioned", condition_mode=condition_mode, agent_type=agent_type))

    def _attach(self):
        return self.sim.direct_pack_rows(only=self.only, reward_weights=self.tracker.reward_weights_tensor)

    @property
    def reward_weights_tensor(self):
        """[W, A, 3] float32: every agent slot's (collision, goal_achieved, off_road) weights, the tracker's tensor."""
        return self.tracker.reward_weights_tensor

    def set_reward_weights(self, worlds=None, condition_mode=None, agent_type=None):
        """New weights for the listed worlds (None: all), `EpisodeTracker.set_reward_weights`; condition_mode None: the
        environment's own mode and agent_type.  The rows' weight columns follow on the device.  Returns
        `reward_weights_tensor`."""
        if condition_mode is None:
            condition_mode, agent_type = self.condition_mode, self.agent_type
        return self.tracker.set_reward_weights(worlds, condition_mode=condition_mode, agent_type=agent_type)
