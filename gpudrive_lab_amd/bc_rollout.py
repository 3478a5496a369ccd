"""The closed-loop BC driver: one episode with the BC policy in the loop, and its metrics, on the device.

`ClosedLoopBC.run()` is the reference's closed-loop script (baselines/il/test/simulation.py run(), lines 22-135): reset the
worlds, keep a window of `num_stack` packed observations per controlled agent, ask the policy for an action for every agent
still alive, write those actions (zeros for everyone else) into the simulator, step, accumulate the off-road / collision /
goal flags, note the step at which goal and off-road first happened and the distance to the goal at the start and at the end,
report the rates.  The reference does this with a dozen eager torch ops, a `cat` of the stacked observation, boolean-mask
gathers (which synchronise) and a scatter per step; here one C call (`gd_bc_rollout`, csrc/bc_rollout.hip) runs the whole
episode on the simulator's stream with no host synchronisation, no allocation and no atomics inside it.

    bc = DeviceBC(sd, max_agents=128, num_stack=5, ...)            # or a DeviceBCPolicy
    loop = ClosedLoopBC(sim, bc.policy)                            # follows the optimiser in place
    ep = loop.run()                                                # 91 steps, deterministic actions
    ep.summary()                                                   # the eight numbers, ONE host read
    ep.goal_step / expert_done_step                                # the reference's normalised goal time is the caller's line

Rows are in `mask.nonzero()` order (default: the controlled agents).  The window handed to the policy, and returned as
`window`, is the one the policy saw at the last iteration that ran.  By default the policy's forward runs on all N rows every
step and a dead row's action is replaced by zeros.  Iterations after every row is dead (the reference's `break`) change no
output; `steps` counts the iterations that exist.

    ep = loop.run(compact=True)                                    # the forward on the rows still alive only
    ep.live_count                                                  # [91] int32: how many that was, per step

`run(compact=True)` is the reference's `obs[~dead]`: per step two more launches list the rows with `dead == 0` on the device
(`gd_live_rows`' kernels on the complement of the byte) and the forward runs on that list (`gd_bc_forward_rows`); the host
never learns the length, so every chunk of `chunk_rows` list positions is still launched and the workgroups past the list
return at their first load.  Every result is `run()`'s bit for bit, except `row_actions` of a dead row: the action of the last
step it was alive at (with `run()`, of the last step).  The row kernel still visits every row -- a dead row's window, masks and
goal distance keep moving in the reference.

    ep = loop.run(attention=True, readout=ro)                      # ro: a bc_readout.ProbeReadout of the policy
    ep.ego_attn_score                                              # [91, N, 4, A - 1] f32: get_context's ego_attn_score per step
    ep.other_pred, ep.ego_pred, ep.ego_pred_prime                  # [91, N, Po, A - 1], [91, N, Pe], [91, N, P] uint8 classes
    ep.world_importance(t)                                         # [W, 4, A] f32: importance_weight.py's scatter for step t

`run(attention=True)` is the reference's baselines/il/test/importance_weight.py: at every step each live agent's ego -> partner
cross-attention weights per head; `run(readout=ro)` is baselines/il/test/intervention.py: at every step the classes pairs of
trained probes read at one layer (`bc_readout`).  Both are written by the episode's one C call (`gd_bc_rollout_readout`): the
head kernel stores the scores from a per-step base pointer, and one launch per chunk right after the tapped layer reads every
probe -- the loop stays one call and no encoder layer runs twice.  The arrays are step-major, like u and z: a step's slice is
contiguous.  A row that is live before step t holds what `policy.context(..., ego_attn_score=)` / `policy.read(...)` give for
that step's window and masks, bit for bit; a row that is dead before step t, and every step whose iteration does not exist,
holds the fill: 0.0 in the scores, 255 in the classes.  With compact=True only live rows are computed, so the fill `run()` made
stays; without it the forward runs on dead rows too: the read-out kernel drops a row whose `dead` byte is set, and one clean-up
launch per step stores 0.0 over the scores the head kernel wrote for dead rows (the head kernel is the plain forward's and is
left alone).  `attention=True` also keeps `dead_mask` (record's), which `world_importance` reads.  Every other field of the
episode is bit-identical to the same `run()` without the two options.

A policy of `network_dim=128` (`DeviceBCPolicy(..., network_dim=128)`, the reference sweep's model) drives the same loop through
`gd_bc_rollout_dim` with the wide forward in it: `run()`, `compact`, `record`, the seeded draw and `attention=True` as above;
`readout=` is a ValueError there (the probes read 64-wide tokens).

Not here: the per-label (TURN / NORMAL / ...) grouping and the CSV, videos / `plot_simulator_state`, `lp_weight.py` (not
runnable in the reference as written), steering the action with the intervened token (the reference only reads
`ego_pred_prime`), fewer launches for the chunks past the list.  The late-fusion PPO policy in such a loop is `ppo_rollout.ClosedLoopPPO`.  `remove_agents_by_id` / `partner_portion_test` are the
caller's `sim.deleteAgents(...)` before `run()`; self-play is a mask with more rows."""
import ctypes as C

import torch

from . import _capi
from .recorder import DYNAMICS_STATE, EPISODE_LEN, ROAD_POINTS, packed_width

WHO = "ClosedLoopBC: "
SUMMARY_NAMES = _capi.BC_ROLLOUT_SUMMARY

# the running state and the results: name -> (dtype, the value run() fills in)
_ROW_ARRAYS = (("dead", torch.uint8, 0), ("goal_achieved", torch.float32, 0), ("off_road", torch.float32, 0),
               ("veh_collision", torch.float32, 0), ("goal_step", torch.int32, -1), ("off_road_step", torch.int32, -1),
               ("init_goal_dist", torch.float32, 0), ("goal_dist", torch.float32, 0))
# the optional per-step records: name -> (columns per (row, step), dtype, default)
_STEP_ARRAYS = (("actions", 3, torch.float32, 0), ("dead_mask", 1, torch.bool, 1), ("ego_global_pos", 2, torch.float32, 0),
                ("ego_global_rot", 1, torch.float32, 0))
_ITEMSIZE = {torch.float32: 4, torch.int32: 4, torch.bool: 1, torch.uint8: 1}


def _check_sim(sim):
    if int(sim._params.dynamicsModel) == DYNAMICS_STATE:
        raise ValueError(WHO + "the State dynamics model's actions have 10 columns; the policy's have 3 (classic, bicycle or "
                         "delta_local)")


def _check_mask(sim, mask):
    if mask is None:
        return
    if not isinstance(mask, torch.Tensor) or mask.dtype != torch.bool or tuple(mask.shape) != (sim._W, sim._A):
        raise ValueError(WHO + "mask must be a [W, A] = [%d, %d] bool tensor, got %s"
                         % (sim._W, sim._A, (tuple(mask.shape), mask.dtype) if isinstance(mask, torch.Tensor) else type(mask)))


def _check_policy(sim, policy):
    from .bc_policy import DeviceBCPolicy
    if not isinstance(policy, DeviceBCPolicy):
        raise ValueError(WHO + "policy must be a DeviceBCPolicy (DeviceBC(...).policy is one), got %s" % type(policy).__name__)
    if policy.max_agents != sim._A:
        raise ValueError(WHO + "policy.max_agents is %d, the simulator's is %d" % (policy.max_agents, sim._A))


def _check_readout(policy, readout):
    if readout is None:
        return
    from .bc_readout import ProbeReadout
    if not isinstance(readout, ProbeReadout):
        raise ValueError(WHO + "readout must be a bc_readout.ProbeReadout, got %s" % type(readout).__name__)
    if readout.policy is not policy:
        raise ValueError(WHO + "readout reads another policy object")


def _check_steps(n_steps):
    if isinstance(n_steps, bool) or not isinstance(n_steps, int) or not 1 <= n_steps <= EPISODE_LEN:
        raise ValueError(WHO + "n_steps must be an int in [1, 91], got %r" % (n_steps,))


class ClosedLoopEpisode:
    """One closed-loop episode, on the device.  N rows in `mask.nonzero()` order:
    goal_achieved / off_road / veh_collision [N] f32 (clamped to 1); goal_step / off_road_step [N] int32 (the raw step index,
    -1: never); init_goal_dist / goal_dist [N] f32; dead [N] bool; steps: the iterations the reference's loop runs before its
    `break` (a 0-d device tensor); window [N, R, D] f32, partner_mask [N, A - 1] bool (`partner_value == 2`), partner_value
    [N, A - 1] uint8 and road_mask [N, 200] bool as the policy last saw them; with record=True actions [N, 91, 3] (zeros once the
    row is dead), dead_mask [N, 91] bool (default 1), ego_global_pos [N, 91, 2] and ego_global_rot [N, 91] (live rows only);
    with attention=True ego_attn_score [91, N, 4, A - 1] f32 (0.0 where the row was dead before the step) and dead_mask; with
    readout= other_pred [91, N, Po, A - 1], ego_pred [91, N, Pe], ego_pred_prime [91, N, P] uint8 (255 where it was dead)."""

    def __init__(self, **arrays):
        self.__dict__.update(arrays)

    def world_importance(self, t):
        """importance_weight.py:75-78 for step t, [W, 4, A] float32, in torch ops on the device with no host read: zeros, and
        in every world with exactly ONE row live before step t, per head, the k-th agent slot (ascending) other than that row's
        own slot receives partner column k of the row's score -- which is the slot that partner column observes (partner j of
        ego slot a is slot j for j < a, j + 1 otherwise).  Needs run(attention=True)."""
        if getattr(self, "ego_attn_score", None) is None:
            raise ValueError(WHO + "world_importance needs run(attention=True)")
        if isinstance(t, bool) or not isinstance(t, int) or not 0 <= t < EPISODE_LEN:
            raise ValueError(WHO + "t must be an int in [0, 91), got %r" % (t,))
        W, A = self.mask.shape
        dev = self.mask.device
        dead = torch.ones(W * A, dtype=torch.bool, device=dev)
        dead[self.row_slot.long()] = self.dead_mask[:, t]
        live = ~dead.view(W, A)
        one = live.sum(dim=1) == 1                                     # [W]
        a = live.to(torch.uint8).argmax(dim=1)                         # [W] the live slot where there is exactly one
        n = self.row_of_slot.view(W, A).gather(1, a[:, None]).squeeze(1).clamp(min=0).long()
        score = self.ego_attn_score[t].index_select(0, n)              # [W, 4, A - 1]
        slot = torch.arange(A, device=dev)[None, :]
        col = (slot - (slot > a[:, None]).long()).clamp(max=A - 2)     # the partner column that observes slot s
        vals = score.gather(2, col[:, None, :].expand(W, 4, A))
        keep = (one[:, None] & (slot != a[:, None]))[:, None, :].expand(W, 4, A)
        return torch.where(keep, vals, torch.zeros((), dtype=torch.float32, device=dev))

    def summary(self):
        """off_road_rate, veh_coll_rate, goal_rate, collision_rate, goal_progress, goal_count, n_rows, iterations as a dict of
        floats: one host read."""
        return dict(zip(SUMMARY_NAMES, (float(v) for v in self.summary_tensor.cpu().tolist())))


class ClosedLoopBC:
    def __init__(self, sim, policy, mask=None):
        """sim: a SimManager (any dynamics model but State).  policy: a `DeviceBCPolicy` with the simulator's max_agents.
        mask: a [W, A] bool tensor of the agent slots the policy drives; default `controlled_state_tensor() == 1`, the
        reference's cont_agent_mask.  Every argument is checked before anything reaches the device (ValueError).  One host
        synchronisation, here, for the number of rows."""
        _check_sim(sim)
        _check_mask(sim, mask)
        _check_policy(sim, policy)
        self.sim, self.policy = sim, policy
        self._explicit = mask is not None
        self._set_rows(mask)

    def _set_rows(self, mask):
        sim = self.sim
        if mask is None:
            mask = sim.controlled_state_tensor().to_torch().squeeze(-1) == 1
        self.mask = mask.to(sim._device).clone()
        self.row_slot = self.mask.reshape(-1).nonzero().squeeze(1).to(torch.int32).contiguous()  # (synchronises)
        self.num_agents = n = int(self.row_slot.shape[0])
        if n < 1:
            raise ValueError(WHO + "the mask selects no agent slot")
        self.row_of_slot = torch.full((sim._W * sim._A,), -1, dtype=torch.int32, device=sim._device)
        self.row_of_slot[self.row_slot.long()] = torch.arange(n, dtype=torch.int32, device=sim._device)

    @staticmethod
    def row_nbytes(max_agents, num_stack, record=False, attention=False, readout=None):
        """Bytes one row takes in a run: the window, both masks, the partner value, the action, the running state and, with
        record, 91 steps of every per-step array.  attention: 91 steps of [4, A - 1] float32 scores (and dead_mask, unless
        record already counts it) -- 46 228 bytes a row at A = 128, so [91, N, 4, 127] is 154 MB at N = 832.  readout (a
        `ProbeReadout`): 91 steps of one byte per class it reads (`readout.row_nbytes()`)."""
        A, R = max_agents, num_stack
        n = R * packed_width(A) * 4 + R * (A - 1) + R * ROAD_POINTS + (A - 1) + 3 * 4
        n += sum(_ITEMSIZE[dt] for _, dt, _ in _ROW_ARRAYS)
        if record:
            n += EPISODE_LEN * sum(c * _ITEMSIZE[dt] for _, c, dt, _ in _STEP_ARRAYS)
        if attention:
            n += EPISODE_LEN * (4 * (A - 1) * 4 + (0 if record else 1))
        if readout is not None:
            n += EPISODE_LEN * readout.row_nbytes()
        return n

    @staticmethod
    def nbytes(sim, policy, record=False, mask=None, stochastic=False, compact=False, attention=False, readout=None):
        """What `run()` will allocate for `sim`, `policy` and `mask` (default: the controlled agents): N rows of `row_nbytes`,
        any_alive [92] int32 and the summary [8]; with stochastic the draws u [91, N] and z [91, N, 3]; with compact the row
        list, its count and scratch (`LiveRows.nbytes(N)`) and live_count [91] int32.  The policy's own blob and scratch are
        the policy's (`policy.nbytes`).  attention / readout: the per-step read-outs, as in `row_nbytes` -- the scores alone are
        [91, N, 4, A - 1] float32, 154 MB at N = 832 and A = 128.  (Synchronises, for N.)"""
        _check_sim(sim)
        _check_mask(sim, mask)
        _check_policy(sim, policy)
        if mask is None:
            mask = sim.controlled_state_tensor().to_torch().squeeze(-1) == 1
        n = int(mask.sum().item())
        _check_readout(policy, readout)
        total = n * ClosedLoopBC.row_nbytes(sim._A, policy.num_stack, record, attention, readout) + (EPISODE_LEN + 1) * 4 \
            + len(SUMMARY_NAMES) * 4
        if stochastic:
            total += EPISODE_LEN * n * 4 * 4
        if compact:
            from .policy import LiveRows
            total += LiveRows.nbytes(n) + EPISODE_LEN * 4
        return total

    def resample(self, scenes):
        """A new batch of scenes: `set_maps`, then the mask (the controlled agents of the new worlds, unless an explicit mask
        was given, which is kept) and the rows derived again."""
        self.sim.set_maps(scenes)
        self._set_rows(self.mask if self._explicit else None)

    @staticmethod
    def _new(name, shape, dtype, fill, device):
        """Every array of a run is made here (fill None: need not be initialised)."""
        return torch.empty(shape, dtype=dtype, device=device) if fill is None else torch.full(shape, fill, dtype=dtype, device=device)

    def run(self, n_steps=EPISODE_LEN, deterministic=True, generator=None, record=False, compact=False, attention=False,
            readout=None):
        """Reset every world, fill the running state and run `n_steps` steps with the policy in the loop in one C call; returns
        the `ClosedLoopEpisode`.  n_steps < 91 gives the prefix of the full episode.  deterministic=False: u [n_steps, N] and
        z [n_steps, N, 3] are drawn from `generator` (a device torch.Generator, required) before the call and consumed per
        step under csrc/bc_rule.hpp's draw; they are returned as `u` and `z`.  record: also keep the per-step arrays.  compact:
        run every step's forward on the list of the rows still alive (`gd_bc_rollout_compact`, see the module docstring); the
        episode then has live_count [91] int32, the length of step t's list, 0 for t >= n_steps, and `live_rows`.  attention:
        also keep ego_attn_score [91, N, 4, A - 1] float32 (and dead_mask); readout: a `bc_readout.ProbeReadout` of the policy,
        whose other_pred / ego_pred / ego_pred_prime are kept as [91, N, ...] uint8 (its labels, if a tensor, are [N] in row
        order); see the module docstring for the fill of dead rows.  Both work with compact and deterministic=False, add one
        launch per chunk and step (and, without compact, one clean-up launch per step for the scores), and change no other
        field.  No host synchronisation."""
        _check_steps(n_steps)
        if readout is not None and getattr(getattr(self, "policy", None), "network_dim", 64) != 64:
            raise ValueError(WHO + "readout= is built at network_dim 64 only, the policy has network_dim %d"
                             % self.policy.network_dim)
        _check_readout(getattr(self, "policy", None), readout)
        deterministic = bool(deterministic)
        if not deterministic and not isinstance(generator, torch.Generator):
            raise ValueError(WHO + "deterministic=False needs generator=, a torch.Generator on the simulator's device")
        sim, pol, n, A, T = self.sim, self.policy, self.num_agents, self.sim._A, EPISODE_LEN
        R, D, dev = pol.num_stack, packed_width(A), sim._device
        if pol.device != dev:
            raise ValueError(WHO + "the policy is on %s, the simulator on %s" % (pol.device, dev))
        b = _capi.GdBCRolloutBuffers()
        out = {}
        b.row_slot, b.row_of_slot, b.n_rows, b.deterministic = self.row_slot.data_ptr(), self.row_of_slot.data_ptr(), n, int(deterministic)
        if not deterministic:
            out["u"] = torch.rand((n_steps, n), dtype=torch.float32, device=dev, generator=generator)
            out["z"] = torch.randn((n_steps, n, 3), dtype=torch.float32, device=dev, generator=generator)
            b.u, b.z = out["u"].data_ptr(), out["z"].data_ptr()
        new = lambda name, shape, dt, fill: self._new(name, shape, dt, fill, dev)
        window = new("window", (n, R, D), torch.float32, None)  # (written before it is read: frames 0..R-2 as zeros at t = 0)
        pm = new("partner_mask", (n, R, A - 1), torch.uint8, 0)
        rm = new("road_mask", (n, R, ROAD_POINTS), torch.uint8, 0)
        pv = new("partner_value", (n, A - 1), torch.uint8, 0)
        row_actions = new("row_actions", (n, 3), torch.float32, 0)
        b.window, b.partner_mask, b.road_mask = window.data_ptr(), pm.data_ptr(), rm.data_ptr()
        b.partner_value, b.row_actions = pv.data_ptr(), row_actions.data_ptr()
        for name, dt, fill in _ROW_ARRAYS:
            out[name] = new(name, (n,), dt, fill)
            setattr(b, name, out[name].data_ptr())
        any_alive = new("any_alive", (T + 1,), torch.int32, 0)
        summary = new("summary", (len(SUMMARY_NAMES),), torch.float32, 0)
        b.any_alive, b.summary = any_alive.data_ptr(), summary.data_ptr()
        if record:
            for name, c, dt, fill in _STEP_ARRAYS:
                out[name] = new(name, (n, T) if c == 1 else (n, T, c), dt, fill)
                setattr(b, name, out[name].data_ptr())
        reads = None
        if attention or readout is not None:
            reads = _capi.GdBCRolloutReads()
            if attention:
                out["ego_attn_score"] = new("ego_attn_score", (T, n, 4, A - 1), torch.float32, 0)
                reads.ego_attn_score = out["ego_attn_score"].data_ptr()
                if not record:
                    out["dead_mask"] = new("dead_mask", (n, T), torch.bool, 1)
                    b.dead_mask = out["dead_mask"].data_ptr()
            if readout is not None:
                from .bc_readout import NO_CLASS
                filled = {name: new(name, (T, n) + readout.row_shape(name), torch.uint8, NO_CLASS) for name in readout.names}
                ro, _ = readout.bind((T, n), filled, who=WHO)
                out.update(filled)
                reads.readout = C.pointer(ro)
        r = None
        if compact:
            from .policy import LiveRows
            out["live_rows"] = lr = LiveRows(n, dev, new=self._new)  # (kept with the episode: the call is still running)
            out["live_count"] = new("live_count", (T,), torch.int32, 0)
            r = _capi.GdBCRolloutRows()
            r.rows, r.count, r.scratch = lr.rows.data_ptr(), lr.count.data_ptr(), lr.scratch.data_ptr()
            r.live_count = out["live_count"].data_ptr()
        sim.reset(list(range(sim._W)))
        sim._bind_stream()
        # The entry and how much of (list, reads) it takes, chosen once.  A 64-wide policy keeps the entry points it had.
        wide = pol.network_dim != 64
        entry, takes = (("gd_bc_rollout_dim", 2) if wide else ("gd_bc_rollout_readout", 2) if reads is not None
                        else ("gd_bc_rollout_compact", 1) if compact else ("gd_bc_rollout", 0))
        p = pol.c_struct_dim() if wide else pol.c_struct()
        tail = (None if r is None else C.byref(r), None if reads is None else C.byref(reads))[:takes]
        _capi.check(getattr(sim._L, entry)(sim._h, C.byref(p), C.byref(b), *tail, n_steps), entry)
        sim._after()
        out["dead"] = out["dead"].view(torch.bool)
        if attention:
            out.update(mask=self.mask, row_slot=self.row_slot, row_of_slot=self.row_of_slot)
        return ClosedLoopEpisode(steps=any_alive[:T].sum(), any_alive=any_alive, summary_tensor=summary, window=window,
                                 partner_mask=pm[:, R - 1].view(torch.bool), road_mask=rm[:, R - 1].view(torch.bool),
                                 partner_value=pv, row_actions=row_actions, **out)
