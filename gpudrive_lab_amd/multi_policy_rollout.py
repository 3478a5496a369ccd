"""The multi-policy closed-loop evaluator: cross-play episodes with several late-fusion policies in the same worlds, on the device.

`ClosedLoopMultiPPO.run()` is the reference's `multi_policy_rollout` (gpudrive/utils/multi_policy_rollout.py:36-154) with its
`compute_metrics` (156-169): every policy owns a [W, A] mask of agents, at every step each policy acts for its agents that are
still live, and the metrics are kept per policy -- how a checkpoint is compared against an earlier one, or a trained policy
against a baseline that shares its scenes.  The reference calls each policy on `next_obs[mask_p & live]` in a Python loop over
the policies, with boolean-mask gathers and scatters that synchronise every step; here one C call (`gd_multi_policy_rollout`)
runs the whole episode on the simulator's stream with no host synchronisation, no allocation and no atomics inside it.  Per
step `gd_owned_rows` turns `live` and the rows' owners into ONE list with a segment per policy, every segment starting at a
multiple of 32, and `gd_policy_forward_owned` runs one forward of three launches on it in which every wave takes the weights of
its segment's policy: 7 launches per step beside the step's own, whatever the number of policies.

    ev = ClosedLoopMultiPPO(eval_sim, {"new": (ppo.policy, mask_a), "old": (baseline, mask_b)}, init_steps=11)
    ep = ev.run(generator=g)                   # 91 steps, sampled actions (the reference's default)
    ep.metrics("new")                          # the reference's nine keys for that policy, on the device
    ep.summary()                               # the totals over all rows and per policy, ONE host read

`policies` is the reference's own argument: an ordered mapping name -> (policy, mask [W, A] bool).  Rows are the simulator's
learner rows, set to the controlled agents; the evaluator attaches its own [N, D] row buffer with only=True and OWNS the
simulator's learner rows, as `ClosedLoopPPO` does.  The fractions divide by the reference's `controlled_per_scene`, the sum over
ALL policies of `mask.sum(dim=1)`: one number per world, not per policy, and it counts every slot a caller put in a mask, also
one that holds no controlled agent.  Such a slot changes nothing else.

Everything `ClosedLoopPPO.run(compact=True)` returns is returned over all rows as well (`PolicyEpisode`): the forward's outputs
of a dead row are those of its last live step.

Not here: rendering / `sim_state_frames` and `center_on_ego`; masks that OVERLAP on a controlled slot (the reference would let
the later policy overwrite the action and count the row for both: refused); `create_data_table`'s pandas tables; BC policies in
the set; dropout (always the unmasked forward: a `DropoutRule` on a policy is neither consulted nor advanced)."""
import ctypes as C

import torch

from . import _capi
from .episode import check_warmup
from .ppo_rollout import (_ROW_ARRAYS, _STEP_ARRAYS, _WORLD_ARRAYS, EVALUATE_COLUMNS, SUMMARY_NAMES, ClosedLoopPPO,
                          PolicyEpisode, _check_action_table, _check_sim, _check_steps, _check_weights)
from .recorder import EPISODE_LEN

WHO = "ClosedLoopMultiPPO: "
MAX_POLICIES = _capi.POLICY_SET_MAX
POLICY_WORLD_RESULTS = _capi.MULTI_POLICY_WORLD       # [P, W] each
POLICY_SUMMARY_NAMES = _capi.MULTI_POLICY_SUMMARY     # per policy
# the reference's nine keys of one policy's metrics (multi_policy_rollout.py:31)
METRIC_KEYS = ("goal_achieved", "collided", "off_road", "off_road_count", "collided_count", "goal_achieved_count", "frac_off_road",
               "frac_collided", "frac_goal_achieved")


def _check_policies(sim, policies):
    """The names, the policies and the masks of `policies`, checked without touching the simulator or a device."""
    from .policy import check_policy_set
    if not isinstance(policies, dict) or not policies:
        raise ValueError(WHO + "policies must be a non-empty dict name -> (DevicePolicy, mask [W, A] bool)")
    if len(policies) > MAX_POLICIES:
        raise ValueError(WHO + "at most %d policies share an episode, got %d" % (MAX_POLICIES, len(policies)))
    names, pols, masks = [], [], []
    for name, entry in policies.items():
        if not isinstance(entry, (tuple, list)) or len(entry) != 2:
            raise ValueError(WHO + "policies[%r] must be a pair (DevicePolicy, mask)" % (name,))
        pol, mask = entry
        if not isinstance(mask, torch.Tensor) or mask.dtype != torch.bool or tuple(mask.shape) != (sim._W, sim._A):
            raise ValueError(WHO + "the mask of %r must be a [W, A] = [%d, %d] bool tensor, got %s"
                             % (name, sim._W, sim._A, (tuple(mask.shape), mask.dtype) if isinstance(mask, torch.Tensor) else type(mask)))
        names.append(name), pols.append(pol), masks.append(mask)
    pols = check_policy_set(pols, WHO)
    if pols[0].max_agents != sim._A:
        raise ValueError(WHO + "the policies' max_agents is %d, the simulator's is %d" % (pols[0].max_agents, sim._A))
    return tuple(names), pols, tuple(masks)


def _owners(controlled, masks):
    """owner [W, A] uint8 (the index of the policy whose mask holds the slot; 255 where no mask does) and the denominator [W]
    float32, on `controlled`'s device.  ValueError when the masks do not cover the controlled slots (the reference's `assert
    torch.all(live_agent_mask == combined_mask)`) or two of them share one."""
    masks = [m.to(controlled.device) for m in masks]
    owner = torch.full(controlled.shape, 255, dtype=torch.uint8, device=controlled.device)
    taken = torch.zeros_like(controlled)
    denominator = torch.zeros(controlled.shape[0], dtype=torch.float32, device=controlled.device)
    for p, m in enumerate(masks):
        mine = m & controlled
        if bool((mine & taken).any()):
            raise ValueError(WHO + "two masks share a controlled slot (policy %d and an earlier one): overlapping masks are "
                             "not built" % p)
        taken |= mine
        owner[mine] = p
        denominator += m.sum(dim=1).float()  # (multi_policy_rollout.py:145: every slot of every mask)
    if not torch.equal(taken, controlled):
        raise ValueError(WHO + "the masks do not cover the controlled agents: %d controlled slots belong to no policy"
                         % int((controlled & ~taken).sum()))
    return owner, denominator


class MultiPolicyEpisode(PolicyEpisode):
    """One multi-policy episode, on the device.  Everything a `PolicyEpisode` of a compact run has, over all N rows, and
    names (the policies, in order); owner [N] uint8, the index of each row's policy; list_count [91, P] int32, the rows of
    policy p live before step t (the lengths of step t's segments; 0 for t >= n_steps); per policy and world [P, W] f32:
    policy_goal_achieved_count / policy_collided_count / policy_off_road_count (the policy's rows in the world whose sum is
    > 0), policy_frac_goal_achieved / policy_frac_collided / policy_frac_off_road (count / denominator, NaN for 0 / 0),
    policy_n_rows; denominator [W] f32; policy_summary_tensor [P, 4]."""

    def metrics(self, name):
        """The reference's nine keys for policy `name`: goal_achieved, collided, off_road as [W, A] float32 (the raw sums of
        the policy's rows, zero in every other slot -- scattered from the rows here), the three counts and the three fractions
        [W].  (The scatter through the boolean mask synchronises, as the reference's does.)"""
        p = self.names.index(name)
        mine = self.owner == p
        out = {}
        for k in ("goal_achieved", "collided", "off_road"):
            grid = torch.zeros(self.mask.shape, dtype=torch.float32, device=self.mask.device)
            grid[self.mask] = torch.where(mine, getattr(self, k), 0.0)
            out[k] = grid
        for k in METRIC_KEYS[3:]:
            out[k] = getattr(self, "policy_" + k)[p]
        return out

    def summary(self):
        """The eight totals over all rows (`PolicyEpisode.summary`) and under "policies" name -> the totals of goal_achieved,
        collided, off_road and n_rows of that policy, as floats: ONE host read."""
        flat = torch.cat([self.summary_tensor, self.policy_summary_tensor.reshape(-1)]).cpu().tolist()
        out = dict(zip(SUMMARY_NAMES, (float(v) for v in flat[:len(SUMMARY_NAMES)])))
        k, rest = len(POLICY_SUMMARY_NAMES), flat[len(SUMMARY_NAMES):]
        out["policies"] = {name: dict(zip(POLICY_SUMMARY_NAMES, (float(v) for v in rest[i * k:(i + 1) * k])))
                           for i, name in enumerate(self.names)}
        return out


class ClosedLoopMultiPPO:
    def __init__(self, sim, policies, action_table=None, init_steps=0, reward_weights=None):
        """sim: a SimManager (classic or bicycle dynamics).  policies: an ordered dict name -> (`DevicePolicy`, mask [W, A]
        bool), 1 to 8 entries; the policies share max_agents (the simulator's), ego_width and n_actions.  action_table,
        init_steps, reward_weights: as for `ClosedLoopPPO`.  The shapes are checked before the simulator or a device is touched
        (ValueError).  Then the controlled agents are read: ValueError when the masks do not cover them, or when two masks
        share a controlled slot.  The learner rows are set to the controlled slots -- one host synchronisation, here -- and the
        [N, D] row buffer is attached with only=True: the evaluator owns the simulator's learner rows."""
        _check_sim(sim)
        self.names, pols, masks = _check_policies(sim, policies)
        _check_weights(sim, pols[0], reward_weights)
        table = _check_action_table(sim, pols[0], action_table)
        check_warmup(init_steps, "reset_worlds")
        from .policy import PolicySet
        self.sim, self.init_steps = sim, int(init_steps)
        self.policy_masks = masks
        controlled = sim.controlled_state_tensor().to_torch().squeeze(-1) == 1
        _owners(controlled, masks)  # (refuses before anything is set)
        self.set = PolicySet(pols)
        self.table = table.to(device=sim._device, dtype=torch.float32).contiguous()
        self.reward_weights = None if reward_weights is None else reward_weights.to(sim._device).contiguous()
        self._set_rows()

    @property
    def policies(self):
        return dict(zip(self.names, self.set.policies))

    def _set_rows(self):
        sim = self.sim
        controlled = sim.controlled_state_tensor().to_torch().squeeze(-1) == 1
        owner, denominator = _owners(controlled, self.policy_masks)
        self.mask = controlled.to(sim._device).clone()
        self.num_agents = n = sim.set_learner_rows(self.mask)  # (synchronises)
        if n < 1:
            raise ValueError(WHO + "no agent is controlled")
        self.owner = owner.to(sim._device)[self.mask].contiguous()
        self.denominator = denominator.to(sim._device).contiguous()
        self.obs = sim.direct_pack_rows(only=True, reward_weights=self.reward_weights)
        self.set._struct(n)  # (the position-indexed scratch of the forward, grown here: run() allocates none of it)

    @staticmethod
    def nbytes(sim, policies, record=False, stochastic=False):
        """What `run()` will allocate for `sim` and `policies`: what `ClosedLoopPPO.nbytes` counts for the controlled agents
        (N rows, W worlds, any_active, the summary, with stochastic the draws), the owned list (`OwnedRows.nbytes(N, P)`),
        list_count [91, P] int32, the seven per-policy results [P, W] and the per-policy summary [P, 4].  The [N, D] row buffer,
        owner [N], the denominator [W] and the forward's position-indexed scratch are the constructor's.  (Synchronises, for
        N.)"""
        from .policy import OwnedRows
        _check_sim(sim)
        names, pols, _ = _check_policies(sim, policies)
        P = len(names)
        n = int((sim.controlled_state_tensor().to_torch().squeeze(-1) == 1).sum().item())
        total = (n * ClosedLoopPPO.row_nbytes(record) + sim._W * ClosedLoopPPO.world_nbytes(sim._A, record)
                 + (EPISODE_LEN + 1) * 4 + len(SUMMARY_NAMES) * 4)
        if stochastic:
            total += EPISODE_LEN * n * 4
        return total + OwnedRows.nbytes(n, P) + EPISODE_LEN * P * 4 + len(POLICY_WORLD_RESULTS) * P * sim._W * 4 \
            + P * len(POLICY_SUMMARY_NAMES) * 4

    def resample(self, scenes):
        """A new batch of scenes: `set_maps`, then the owners, the denominator, the learner rows and the row buffer derived
        again from the same masks, which must cover the controlled agents of the new worlds (ValueError otherwise)."""
        self.sim.set_maps(scenes)
        self._set_rows()

    _new = staticmethod(ClosedLoopPPO._new)

    def run(self, n_steps=EPISODE_LEN, deterministic=False, generator=None, record=False):
        """Reset every world, advance the log playback by init_steps, and run `n_steps` steps with the policies in the loop in
        ONE C call; returns the `MultiPolicyEpisode`.  n_steps < 91 gives the prefix of the full episode.
        deterministic=False (the reference's default): u [n_steps, N] is drawn from `generator` (a device torch.Generator,
        required) before the call, step t consumes u[t] under csrc/policy_rule.hpp's draw -- a row takes its own u whichever
        policy owns it -- and it is returned as `u`; deterministic=True takes the first index of the largest logit.  record:
        also keep the per-step arrays.  No host synchronisation."""
        _check_steps(n_steps)
        deterministic = bool(deterministic)
        if not deterministic and not isinstance(generator, torch.Generator):
            raise ValueError(WHO + "deterministic=False needs generator=, a torch.Generator on the simulator's device")
        from .policy import OwnedRows
        sim, ps, n, T = self.sim, self.set, self.num_agents, EPISODE_LEN
        W, A, dev, P = sim._W, sim._A, sim._device, len(self.names)
        if ps.device != dev:
            raise ValueError(WHO + "the policies are on %s, the simulator on %s" % (ps.device, dev))
        b, m = _capi.GdPolicyRolloutBuffers(), _capi.GdMultiPolicyBuffers()
        out = {}
        b.n_rows, b.deterministic, b.table, b.n_actions = n, int(deterministic), self.table.data_ptr(), int(self.table.shape[0])
        if not deterministic:
            out["u"] = torch.rand((n_steps, n), dtype=torch.float32, device=dev, generator=generator)
            b.u = out["u"].data_ptr()
        new = lambda name, shape, dt, fill: self._new(name, shape, dt, fill, dev)  # noqa: E731
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
        out["owned_rows"] = lr = OwnedRows(n, P, dev, new=self._new)  # (kept with the episode: the call is still running)
        out["list_count"] = new("list_count", (T, P), torch.int32, 0)
        m.owner, m.denominator = self.owner.data_ptr(), self.denominator.data_ptr()
        m.rows, m.start, m.count, m.scratch = lr.rows.data_ptr(), lr.start.data_ptr(), lr.count.data_ptr(), lr.scratch.data_ptr()
        m.list_count = out["list_count"].data_ptr()
        for name in POLICY_WORLD_RESULTS:
            out["policy_" + name] = new("policy_" + name, (P, W), torch.float32, 0)
            setattr(m, name, out["policy_" + name].data_ptr())
        policy_summary = new("policy_summary", (P, len(POLICY_SUMMARY_NAMES)), torch.float32, 0)
        m.summary = policy_summary.data_ptr()
        s = ps._struct(n)
        sim.reset(list(range(W)))
        if self.init_steps > 0:
            sim.advance_log_playback(self.init_steps)
        sim._bind_stream()
        _capi.check(sim._L.gd_multi_policy_rollout(sim._h, C.byref(s), C.byref(b), C.byref(m), n_steps), "gd_multi_policy_rollout")
        sim._after()
        out["live"] = out["live"].view(torch.bool)
        out["world_active"] = out["world_active"].view(torch.bool)
        return MultiPolicyEpisode(steps=any_active[:n_steps].sum(), any_active=any_active, summary_tensor=summary,
                                  policy_summary_tensor=policy_summary, names=self.names, owner=self.owner, mask=self.mask,
                                  denominator=self.denominator, **out)

    def evaluate(self, scene_batches, n_steps=EPISODE_LEN, deterministic=False, generator=None):
        """`ClosedLoopPPO.evaluate` with the policies in the loop: for every batch of scenes `resample(batch)` and `run()`.
        Returns the same dict (the reference's column names over all rows -> float32 numpy arrays of one entry per world and
        batch, and "scene") and under "policies" name -> {the six per-policy counts and fractions -> such arrays}; all
        results are read back together, in ONE host read at the end."""
        scenes, cols = [], []
        for batch in scene_batches:
            batch = list(batch)
            self.resample(batch)
            ep = self.run(n_steps=n_steps, deterministic=deterministic, generator=generator)
            scenes.extend(batch)
            cols.append(torch.cat([torch.stack([getattr(ep, src) for _, src in EVALUATE_COLUMNS])]
                                  + [getattr(ep, "policy_" + k) for k in METRIC_KEYS[3:]]))
        if not cols:
            raise ValueError(WHO + "evaluate: no batch of scenes")
        table = torch.cat(cols, dim=1).cpu().numpy()
        res = {"scene": scenes}
        res.update((name, table[i]) for i, (name, _) in enumerate(EVALUATE_COLUMNS))
        at, P = len(EVALUATE_COLUMNS), len(self.names)
        res["policies"] = {name: {k: table[at + j * P + p] for j, k in enumerate(METRIC_KEYS[3:])}
                           for p, name in enumerate(self.names)}
        return res
