"""The closed-loop PPO evaluator: one episode with the late-fusion policy in the loop, and its per-world metrics, on the device.

`ClosedLoopPPO.run()` is the reference's evaluation rollout (examples/experimental/eval_utils.py rollout(), lines 94-227): reset
the worlds, ask the policy for a discrete action index for every controlled agent still live, decode the indices through the
action table (index 0 for everyone else), step, add the off-road / collision / goal flags of the live rows, retire the rows
that are done, note the step at which every world finished, and report per world how many rows achieved the goal, collided,
went off road or did none of the three, as counts and as fractions of the world's rows.  `evaluate()` is the loop of
`evaluate_policy()` around it (lines 283-358): a new batch of scenes, a rollout, the per-world results concatenated.  The
reference does this with boolean-mask gathers and scatters, which synchronise every step, and a Python loop over the worlds;
here one C call (`gd_policy_rollout`, csrc/policy_rollout.hip) runs the whole episode on the simulator's stream with no host
synchronisation, no allocation and no atomics inside it.

    ppo = DevicePPO(sd, max_agents=128, ...)                       # or a DevicePolicy
    ev = ClosedLoopPPO(eval_sim, ppo.policy, init_steps=11)        # follows the optimiser in place
    ep = ev.run(generator=g)                                       # 91 steps, sampled actions (the reference's default)
    ep.summary()                                                   # the eight numbers, ONE host read
    ep.frac_goal_achieved, ep.episode_lengths                      # [W], on the device
    res = ev.evaluate(scene_batches, generator=g)                  # one host read at the end

Rows are the simulator's learner rows, in `mask.nonzero()` order (default: the controlled agents): the evaluator sets them
and attaches its own [N, D] row buffer with only=True, so it OWNS the simulator's learner rows.  A simulator serves one of
`DeviceLearnerEnv` / `ClosedLoopPPO` at a time; evaluation normally has its own simulator, on held-out scenes.  The forward is
always the unmasked one (the reference's `load_policy` returns `policy.eval()`): a `DropoutRule` on the policy is neither
consulted nor advanced.  By default it runs on all N rows every step and a dead row's index is replaced by 0;
`run(compact=True)` puts the list of live rows in the loop instead (`gd_policy_rollout_compact`: per step `gd_live_rows` on
`live`, then the forward on that list), so a step costs what its live rows cost.  Every result is the same bit for bit, except
that `actions`, `logprob`, `entropy` and `value` of a dead row are those of its last live step, and the episode gains
`live_count` [91].  It is opt-in.
Iterations after every world is done (the reference's `break`) change no output; `steps` counts the iterations that exist.

Several policies in the same worlds (the reference's `multi_policy_rollout.py`) are `multi_policy_rollout.ClosedLoopMultiPPO`.
Not here: rendering / `sim_state_frames` and `center_on_ego`, the
delta_local table (8000 actions is beyond `DevicePolicy`'s 1024), the CSV / dataframe of `evaluate_policy` (`evaluate()`
returns the columns as numpy arrays)."""
import ctypes as C

import torch

from . import _capi
from .episode import check_warmup
from .learner import _DYNAMICS_NAMES, _check_table
from .learner import action_table as _default_table
from .recorder import DYNAMICS_STATE, EPISODE_LEN

WHO = "ClosedLoopPPO: "
SUMMARY_NAMES = _capi.POLICY_ROLLOUT_SUMMARY

# the forward's outputs and the running state per row: name -> (dtype, the value run() fills in; None: need not be initialised)
_ROW_ARRAYS = (("actions", torch.int64, None), ("logprob", torch.float32, None), ("entropy", torch.float32, None),
               ("value", torch.float32, None), ("live", torch.uint8, 1), ("goal_achieved", torch.float32, 0),
               ("collided", torch.float32, 0), ("off_road", torch.float32, 0))
# the running state and the results per world
WORLD_RESULTS = ("goal_achieved_count", "frac_goal_achieved", "collided_count", "frac_collided", "off_road_count", "frac_off_road",
                 "other_count", "frac_other", "controlled_per_scene")
_WORLD_ARRAYS = ((("world_active", torch.uint8, 1), ("episode_lengths", torch.float32, 0), ("bad_indices", torch.int32, 0))
                 + tuple((name, torch.float32, 0) for name in WORLD_RESULTS))
# the optional per-step records per row: name -> (dtype, default)
_STEP_ARRAYS = (("actions_idx", torch.int64, -1), ("live_mask", torch.bool, 0))
_ITEMSIZE = {torch.float32: 4, torch.int32: 4, torch.int64: 8, torch.bool: 1, torch.uint8: 1}
# evaluate()'s columns, by the reference's names (eval_utils.py:294-306), and where each comes from
EVALUATE_COLUMNS = (("goal_achieved_count", "goal_achieved_count"), ("goal_achieved_frac", "frac_goal_achieved"),
                    ("collided_count", "collided_count"), ("collided_frac", "frac_collided"),
                    ("off_road_count", "off_road_count"), ("off_road_frac", "frac_off_road"), ("other_count", "other_count"),
                    ("other_frac", "frac_other"), ("controlled_agents_in_scene", "controlled_per_scene"),
                    ("episode_lengths", "episode_lengths"))


def _check_sim(sim):
    if int(sim._params.dynamicsModel) == DYNAMICS_STATE:
        raise ValueError(WHO + "the State dynamics model has no discrete action space (classic or bicycle)")


def _check_mask(sim, mask):
    if mask is None:
        return
    if not isinstance(mask, torch.Tensor) or mask.dtype != torch.bool or tuple(mask.shape) != (sim._W, sim._A):
        raise ValueError(WHO + "mask must be a [W, A] = [%d, %d] bool tensor, got %s"
                         % (sim._W, sim._A, (tuple(mask.shape), mask.dtype) if isinstance(mask, torch.Tensor) else type(mask)))


def _check_policy(sim, policy):
    from .policy import DevicePolicy
    if not isinstance(policy, DevicePolicy):
        raise ValueError(WHO + "policy must be a DevicePolicy (DevicePPO(...).policy is one), got %s" % type(policy).__name__)
    if policy.max_agents != sim._A:
        raise ValueError(WHO + "policy.max_agents is %d, the simulator's is %d" % (policy.max_agents, sim._A))


def _check_weights(sim, policy, reward_weights):
    if policy.ego_width == 9:
        wt = reward_weights
        if not isinstance(wt, torch.Tensor) or wt.dtype != torch.float32 or tuple(wt.shape) != (sim._W, sim._A, 3):
            raise ValueError(WHO + "an ego_width 9 policy reads reward-conditioned rows: reward_weights must be a [W, A, 3] = "
                             "[%d, %d, 3] float32 tensor, got %s"
                             % (sim._W, sim._A, (tuple(wt.shape), wt.dtype) if isinstance(wt, torch.Tensor) else type(wt)))
    elif reward_weights is not None:
        raise ValueError(WHO + "reward_weights belongs to an ego_width 9 policy; this policy's ego_width is %d" % policy.ego_width)


def _check_action_table(sim, policy, table):
    """The table run() will use, on the host: the given one, or the default of the simulator's dynamics model."""
    _check_table("ClosedLoopPPO", table)
    if table is None:
        model = _DYNAMICS_NAMES[int(sim._params.dynamicsModel)]
        if model == "delta_local":
            raise ValueError(WHO + "the delta_local table has 8000 actions, a DevicePolicy at most 1024: not built")
        table = _default_table(model)
    if int(table.shape[0]) != policy.n_actions:
        raise ValueError(WHO + "action_table has %d rows, the policy's n_actions is %d" % (table.shape[0], policy.n_actions))
    return table


def _check_steps(n_steps):
    if isinstance(n_steps, bool) or not isinstance(n_steps, int) or not 1 <= n_steps <= EPISODE_LEN:
        raise ValueError(WHO + "n_steps must be an int in [1, 91], got %r" % (n_steps,))


def _check_args(sim, policy, mask, action_table, init_steps, reward_weights):
    _check_sim(sim)
    _check_mask(sim, mask)
    _check_policy(sim, policy)
    _check_weights(sim, policy, reward_weights)
    table = _check_action_table(sim, policy, action_table)
    check_warmup(init_steps, "reset_worlds")
    return table


class PolicyEpisode:
    """One closed-loop episode, on the device.  W worlds, N rows in `mask.nonzero()` order:
    goal_achieved_count / collided_count / off_road_count / other_count [W] f32: the world's rows whose sum is > 0 (other: all
    three == 0); frac_goal_achieved / frac_collided / frac_off_road / frac_other [W] f32: count / controlled_per_scene, NaN
    for a world without rows; controlled_per_scene [W] f32; episode_lengths [W] f32: the first step at which every row of the
    world was done (0 if that never happened, as in the reference).  goal_achieved / collided / off_road [N] f32: the raw sums
    over the steps the row was live (not clamped); live [N] bool.  steps: the iterations the reference's loop runs before its
    `break` (a 0-d device tensor); any_active [92].  actions / logprob / entropy / value [N]: the last forward's outputs.
    With deterministic=False u [n_steps, N].  With record=True actions_idx [N, 91] int64 (-1 once the row is dead, and for
    iterations that do not exist), live_mask [N, 91] bool (live before step t) and agent_positions [W, A, 91, 2] (the
    absolute position of every slot after step t).  With compact=True live_count [91] int32: the rows live before step t, the
    length of the list step t's forward ran on, and live_rows, the `LiveRows` the call used (the last step's list); actions /
    logprob / entropy / value of a dead row are its last live step's."""

    def __init__(self, **arrays):
        self.__dict__.update(arrays)

    def summary(self):
        """The totals of goal_achieved, collided, off_road and other, n_rows, worlds_with_rows, iterations and
        mean_episode_length as a dict of floats: one host read."""
        return dict(zip(SUMMARY_NAMES, (float(v) for v in self.summary_tensor.cpu().tolist())))


class ClosedLoopPPO:
    def __init__(self, sim, policy, mask=None, action_table=None, init_steps=0, reward_weights=None):
        """sim: a SimManager (classic or bicycle dynamics).  policy: a `DevicePolicy` with the simulator's max_agents.  mask: a
        [W, A] bool tensor of the agent slots the policy drives; default `controlled_state_tensor() == 1`, the reference's
        cont_agent_mask.  action_table: float32 [n_actions, 3], default `learner.action_table()` of the simulator's dynamics
        model; its rows must be the policy's n_actions.  init_steps: the reference's warm-up, 0..90: every `run()` advances
        the worlds that many steps with the logged actions after the reset (its env.reset does).  reward_weights: the
        [W, A, 3] float32 weights of a reward-conditioned policy (ego_width 9: required; ego_width 6: refused).  Every
        argument is checked before the simulator or the device is touched (ValueError).  Then the learner rows are set from
        the mask -- one host synchronisation, here, for the number of rows -- and the [N, D] row buffer is attached with
        only=True: the evaluator owns the simulator's learner rows (see the module docstring)."""
        table = _check_args(sim, policy, mask, action_table, init_steps, reward_weights)
        self.sim, self.policy, self.init_steps = sim, policy, int(init_steps)
        self.table = table.to(device=sim._device, dtype=torch.float32).contiguous()
        self.reward_weights = None if reward_weights is None else reward_weights.to(sim._device).contiguous()
        self._explicit = mask is not None
        self._set_rows(mask)

    def _set_rows(self, mask):
        sim = self.sim
        if mask is None:
            mask = sim.controlled_state_tensor().to_torch().squeeze(-1) == 1
        self.mask = mask.to(sim._device).clone()
        self.num_agents = n = sim.set_learner_rows(self.mask)  # (synchronises)
        if n < 1:
            raise ValueError(WHO + "the mask selects no agent slot")
        self.obs = sim.direct_pack_rows(only=True, reward_weights=self.reward_weights)

    @staticmethod
    def row_nbytes(record=False):
        """Bytes one row takes in a run: the forward's four outputs, live and the three sums; with record 91 steps of
        actions_idx and live_mask."""
        n = sum(_ITEMSIZE[dt] for _, dt, _ in _ROW_ARRAYS)
        if record:
            n += EPISODE_LEN * sum(_ITEMSIZE[dt] for _, dt, _ in _STEP_ARRAYS)
        return n

    @staticmethod
    def world_nbytes(max_agents, record=False):
        """Bytes one world takes in a run: world_active, episode_lengths, bad_indices and the nine results; with record
        agent_positions of its `max_agents` slots."""
        n = sum(_ITEMSIZE[dt] for _, dt, _ in _WORLD_ARRAYS)
        if record:
            n += max_agents * EPISODE_LEN * 2 * 4
        return n

    @staticmethod
    def nbytes(sim, policy, record=False, mask=None, stochastic=False, compact=False):
        """What `run()` will allocate for `sim`, `policy` and `mask` (default: the controlled agents): N rows of `row_nbytes`,
        W worlds of `world_nbytes`, any_active [92] int32 and the summary [8]; with stochastic the draws u [91, N]; with
        compact the row list, its count and scratch (`LiveRows.nbytes(N)`) and live_count [91] int32.  The
        [N, D] row buffer is the constructor's, the blob and the features / logits scratch the policy's.  (Synchronises,
        for N.)"""
        _check_sim(sim)
        _check_mask(sim, mask)
        _check_policy(sim, policy)
        if mask is None:
            mask = sim.controlled_state_tensor().to_torch().squeeze(-1) == 1
        n = int(mask.sum().item())
        total = (n * ClosedLoopPPO.row_nbytes(record) + sim._W * ClosedLoopPPO.world_nbytes(sim._A, record)
                 + (EPISODE_LEN + 1) * 4 + len(SUMMARY_NAMES) * 4)
        if stochastic:
            total += EPISODE_LEN * n * 4
        if compact:
            from .policy import LiveRows
            total += LiveRows.nbytes(n) + EPISODE_LEN * 4
        return total

    def resample(self, scenes):
        """A new batch of scenes: `set_maps`, then the mask (the controlled agents of the new worlds, unless an explicit mask
        was given, which is kept), the learner rows and the row buffer derived again."""
        self.sim.set_maps(scenes)
        self._set_rows(self.mask if self._explicit else None)

    @staticmethod
    def _new(name, shape, dtype, fill, device):
        """Every array of a run is made here (fill None: need not be initialised)."""
        return torch.empty(shape, dtype=dtype, device=device) if fill is None else torch.full(shape, fill, dtype=dtype, device=device)

    def run(self, n_steps=EPISODE_LEN, deterministic=False, generator=None, record=False, compact=False):
        """Reset every world, advance the log playback by init_steps, and run `n_steps` steps with the policy in the loop in
        ONE C call; returns the `PolicyEpisode`.  n_steps < 91 gives the prefix of the full episode.  deterministic=False (the
        reference's default): u [n_steps, N] is drawn from `generator` (a device torch.Generator, required) before the call,
        step t consumes u[t] under csrc/policy_rule.hpp's draw, and it is returned as `u`; deterministic=True takes the
        first index of the largest logit.  record: also keep the per-step arrays.  compact: run every step's forward on the
        list of the rows still live (see the module docstring); the episode then has live_count [91] int32, the length of step
        t's list, 0 for t >= n_steps.  No host synchronisation."""
        _check_steps(n_steps)
        deterministic = bool(deterministic)
        if not deterministic and not isinstance(generator, torch.Generator):
            raise ValueError(WHO + "deterministic=False needs generator=, a torch.Generator on the simulator's device")
        sim, pol, n, T = self.sim, self.policy, self.num_agents, EPISODE_LEN
        W, A, dev = sim._W, sim._A, sim._device
        if pol.device != dev:
            raise ValueError(WHO + "the policy is on %s, the simulator on %s" % (pol.device, dev))
        b = _capi.GdPolicyRolloutBuffers()
        out = {}
        b.n_rows, b.deterministic, b.table, b.n_actions = n, int(deterministic), self.table.data_ptr(), int(self.table.shape[0])
        if not deterministic:
            out["u"] = torch.rand((n_steps, n), dtype=torch.float32, device=dev, generator=generator)
            b.u = out["u"].data_ptr()
        new = lambda name, shape, dt, fill: self._new(name, shape, dt, fill, dev)
        for name, dt, fill in _ROW_ARRAYS:
            out[name] = new(name, (n,), dt, fill)
            setattr(b, name, out[name].data_ptr())
        for name, dt, fill in _WORLD_ARRAYS:
            out[name] = new(name, (W,), dt, fill)
            setattr(b, name, out[name].data_ptr())
        any_active = new("any_active", (T + 1,), torch.int32, 0)
        any_active[0:1].fill_(1)  # iteration 0 always exists (a fill: an indexed assignment of a scalar synchronises)
        summary = new("summary", (len(SUMMARY_NAMES),), torch.float32, 0)
        b.any_active, b.summary = any_active.data_ptr(), summary.data_ptr()
        if record:
            for name, dt, fill in _STEP_ARRAYS:
                out[name] = new(name, (n, T), dt, fill)
                setattr(b, name, out[name].data_ptr())
            out["agent_positions"] = new("agent_positions", (W, A, T, 2), torch.float32, 0)
            b.agent_positions = out["agent_positions"].data_ptr()
        p = pol._struct(n)  # (the policy's own scratch, grown to N by the policy's own rule)
        if compact:
            from .policy import LiveRows
            out["live_rows"] = lr = LiveRows(n, dev, new=self._new)  # (kept with the episode: the call is still running)
            out["live_count"] = new("live_count", (T,), torch.int32, 0)
            r = _capi.GdPolicyRolloutRows()
            r.rows, r.count, r.scratch = lr.rows.data_ptr(), lr.count.data_ptr(), lr.scratch.data_ptr()
            r.live_count = out["live_count"].data_ptr()
        sim.reset(list(range(W)))
        if self.init_steps > 0:
            sim.advance_log_playback(self.init_steps)
        sim._bind_stream()
        if compact:
            _capi.check(sim._L.gd_policy_rollout_compact(sim._h, C.byref(p), C.byref(b), C.byref(r), n_steps),
                        "gd_policy_rollout_compact")
        else:
            _capi.check(sim._L.gd_policy_rollout(sim._h, C.byref(p), C.byref(b), n_steps), "gd_policy_rollout")
        sim._after()
        out["live"] = out["live"].view(torch.bool)
        out["world_active"] = out["world_active"].view(torch.bool)
        return PolicyEpisode(steps=any_active[:n_steps].sum(), any_active=any_active, summary_tensor=summary, **out)

    def evaluate(self, scene_batches, n_steps=EPISODE_LEN, deterministic=False, generator=None, compact=False):
        """The loop of the reference's `evaluate_policy` (eval_utils.py:308-358): for every batch of scenes (each a list of W
        paths) `resample(batch)` and `run()`, the per-world results concatenated in batch order.  Returns a dict of the
        reference's column names -> float32 numpy arrays of one entry per world and batch, and "scene" -> the paths; all
        results are read back together, in ONE host read at the end (`resample` synchronises once per batch, for the rows).
        compact: every `run()` with the list of live rows in the loop; the columns are the same."""
        scenes, cols = [], []
        for batch in scene_batches:
            batch = list(batch)
            self.resample(batch)
            ep = self.run(n_steps=n_steps, deterministic=deterministic, generator=generator, compact=compact)
            scenes.extend(batch)
            cols.append(torch.stack([getattr(ep, src) for _, src in EVALUATE_COLUMNS]))
        if not cols:
            raise ValueError(WHO + "evaluate: no batch of scenes")
        table = torch.cat(cols, dim=1).cpu().numpy()
        res = {"scene": scenes}
        res.update((name, table[i]) for i, (name, _) in enumerate(EVALUATE_COLUMNS))
        return res
