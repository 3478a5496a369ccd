"""The expert trajectory recorder: the imitation-learning dataset written on the device.

`ExpertRecorder.record()` is the reference's `save_trajectory` (gpudrive/integrations/il/storage.py:10-109): it replays one
episode with the logged actions and keeps, per controlled agent and time step, the packed observation, the action fed, the
dead / partner / road masks and the global pose -- the arrays baselines/il/il.py:71-84 trains from.  The reference fills them
with a Python loop over every controlled agent inside a loop over 91 steps (storage.py:47-56); here one C call
(`gd_record_expert`) launches one kernel per time index between the steps and leaves the whole dataset in device memory, with
no host synchronisation inside the episode.  `ExpertEpisode.save()` is the one place that leaves the device.

The recorder does not chunk: `ExpertRecorder.nbytes()` tells a caller what a batch will allocate, so it can size W."""
import ctypes as C
import os

import torch

from . import _capi

EPISODE_LEN = 91
ROAD_POINTS = 200
DYNAMICS_STATE = 3


def packed_width(max_agents):
    """D of the packed observation: ego 6 | partners (A - 1) x 6 | road points 200 x 13."""
    return 6 + (max_agents - 1) * 6 + ROAD_POINTS * 13


# name -> (columns per (row, step) as a function of A, dtype, the default of storage.py:29-35)
_STEP_ARRAYS = (
    ("obs", packed_width, torch.float32, 0),
    ("actions", lambda A: 3, torch.float32, 0),
    ("dead_mask", lambda A: 1, torch.bool, 1),
    ("partner_mask", lambda A: A - 1, torch.uint8, 2),
    ("road_mask", lambda A: ROAD_POINTS, torch.bool, 1),
    ("ego_global_pos", lambda A: 2, torch.float32, 0),
    ("ego_global_rot", lambda A: 1, torch.float32, 0),
)
_ROW_ARRAYS = (("dead", torch.uint8), ("goal_achieved", torch.float32), ("off_road", torch.float32),
               ("veh_collision", torch.float32))
_ITEMSIZE = {torch.float32: 4, torch.bool: 1, torch.uint8: 1}


def _check_model(sim):
    if int(sim._params.dynamicsModel) == DYNAMICS_STATE:
        raise ValueError("ExpertRecorder: the State dynamics model's actions have 10 columns; the dataset's have 3 "
                         "(classic, bicycle or delta_local)")


def _check_mask(sim, mask):
    if mask is None:
        return
    if not isinstance(mask, torch.Tensor) or mask.dtype != torch.bool or tuple(mask.shape) != (sim._W, sim._A):
        raise ValueError("ExpertRecorder: mask must be a [W, A] = [%d, %d] bool tensor, got %s"
                         % (sim._W, sim._A, (tuple(mask.shape), mask.dtype) if isinstance(mask, torch.Tensor) else type(mask)))


class ExpertEpisode:
    """One recorded episode, on the device.  N rows in `mask.nonzero()` order:
    obs [N, 91, D] f32, actions [N, 91, 3] f32, dead_mask [N, 91] bool, partner_mask [N, 91, A - 1] uint8,
    road_mask [N, 91, 200] bool, ego_global_pos [N, 91, 2] f32, ego_global_rot [N, 91, 1] f32,
    goal_achieved / off_road / veh_collision [N] f32 (clamped to 1), keep [N] bool = ~((veh_collision + off_road) > 0)
    (storage.py:86-98), steps: the iterations the reference's loop runs before its `break` (a 0-d device tensor)."""

    ARRAYS = tuple(a[0] for a in _STEP_ARRAYS)

    def __init__(self, obs, actions, dead_mask, partner_mask, road_mask, ego_global_pos, ego_global_rot, goal_achieved,
                 off_road, veh_collision, steps):
        self.obs, self.actions, self.dead_mask = obs, actions, dead_mask
        self.partner_mask, self.road_mask = partner_mask, road_mask
        self.ego_global_pos, self.ego_global_rot = ego_global_pos, ego_global_rot
        self.goal_achieved, self.off_road, self.veh_collision = goal_achieved, off_road, veh_collision
        self.keep = ~((veh_collision + off_road) > 0)
        self.steps = steps

    def save(self, path, index=0):
        """Write `path/trajectory_{index}.npz` (obs, actions, dead_mask, partner_mask, road_mask) and
        `path/global/global_trajectory_{index}.npz` (ego_global_pos, ego_global_rot) with the reference's keys and dtypes
        (float32; masks bool; partner_mask int64), the `keep` rows only (storage.py:91-109).  Returns the two file names."""
        import numpy as np
        keep = self.keep
        host = lambda x: x[keep].cpu().numpy()
        os.makedirs(os.path.join(path, "global"), exist_ok=True)
        main = os.path.join(path, "trajectory_%s.npz" % index)
        glob = os.path.join(path, "global", "global_trajectory_%s.npz" % index)
        np.savez_compressed(main, obs=host(self.obs), actions=host(self.actions), dead_mask=host(self.dead_mask),
                            partner_mask=host(self.partner_mask).astype(np.int64), road_mask=host(self.road_mask))
        np.savez_compressed(glob, ego_global_pos=host(self.ego_global_pos), ego_global_rot=host(self.ego_global_rot))
        return main, glob

    def dataset(self, **kw):
        """The `DeviceExpertDataset` over this episode where it lies (il_dataset.py; rollout_len = 5, pred_len = 1)."""
        from .il_dataset import DeviceExpertDataset
        return DeviceExpertDataset(self, **kw)

    def future_dataset(self, **kw):
        """The `DeviceFutureDataset` over this episode where it lies: linear-probing batches with future position labels
        (il_dataset.py; rollout_len = 5, pred_len = 1, future_step = 1, exp = 'other')."""
        from .il_dataset import DeviceFutureDataset
        return DeviceFutureDataset(self, **kw)


class ExpertRecorder:
    def __init__(self, sim, mask=None):
        """sim: a SimManager (any dynamics model but State).  mask: a [W, A] bool tensor of the agent slots to record;
        default `controlled_state_tensor() == 1`, the reference's cont_agent_mask.  Rows are in `mask.nonzero()` order.
        The arguments and the dynamics model are checked before anything reaches the device (ValueError).  One host
        synchronisation, here, for the number of rows."""
        _check_model(sim)
        _check_mask(sim, mask)
        self.sim = sim
        self._explicit = mask is not None
        self._set_rows(mask)

    def _set_rows(self, mask):
        sim = self.sim
        if mask is None:
            mask = sim.controlled_state_tensor().to_torch().squeeze(-1) == 1
        self.mask = mask.to(sim._device).clone()
        self.row_slot = self.mask.reshape(-1).nonzero().squeeze(1).to(torch.int32).contiguous()  # (synchronises)
        self.num_agents = int(self.row_slot.shape[0])

    @staticmethod
    def row_nbytes(max_agents):
        """Bytes one recorded row takes: 91 steps of every array plus the running state."""
        per_step = sum(cols(max_agents) * _ITEMSIZE[dt] for _, cols, dt, _ in _STEP_ARRAYS)
        return EPISODE_LEN * per_step + sum(_ITEMSIZE[dt] for _, dt in _ROW_ARRAYS)

    @staticmethod
    def nbytes(sim, mask=None):
        """What `record()` will allocate for `sim` and `mask` (default: the controlled agents): 91 x N x about 12 KB at 64
        agent slots, 14 KB at 128.  The recorder does not chunk; size W by this.  (Synchronises, for N.)"""
        _check_mask(sim, mask)
        if mask is None:
            mask = sim.controlled_state_tensor().to_torch().squeeze(-1) == 1
        return int(mask.sum().item()) * ExpertRecorder.row_nbytes(sim._A) + (EPISODE_LEN + 1) * 4

    def resample(self, scenes):
        """A new batch of scenes: `set_maps`, then the mask (the controlled agents of the new worlds, unless the recorder
        was given an explicit mask, which is kept) and the rows derived again."""
        self.sim.set_maps(scenes)
        self._set_rows(self.mask if self._explicit else None)

    def record(self, n_steps=EPISODE_LEN, buffers=None, time_kernel=False):
        """Reset every world, fill the defaults (storage.py:29-35), replay `n_steps` logged steps in one C call and return
        the `ExpertEpisode`.  No host synchronisation.  n_steps < 91 gives the prefix [0, n_steps) of the full recording.
        buffers: optional dict name -> flat device tensor to record into (any of `ExpertEpisode.ARRAYS`; at least
        N * 91 * columns elements of the array's dtype); default: fresh allocations.  time_kernel: also measure the
        recorder kernel's launches with events (`last_kernel_ms`; this synchronises)."""
        sim, n, A, T = self.sim, self.num_agents, self.sim._A, EPISODE_LEN
        if not 1 <= int(n_steps) <= T:
            raise ValueError("ExpertRecorder.record: n_steps must be in [1, 91], got %r" % (n_steps,))
        dev = sim._device
        m = max(n, 1)  # (real allocations for n = 0)
        b = _capi.GdRecordBuffers()
        out = {}
        for name, cols, dt, default in _STEP_ARRAYS:
            c = cols(A)
            buf = None if buffers is None else buffers.get(name)
            if buf is None:
                buf = torch.empty((m * T * c,), dtype=dt, device=dev)
            if not (buf.is_cuda and buf.is_contiguous() and buf.dtype == dt and buf.numel() >= m * T * c):
                raise ValueError("ExpertRecorder.record: buffers[%r] must be a contiguous device %s tensor of >= %d elements"
                                 % (name, dt, m * T * c))
            view = buf.view(-1)[:n * T * c]
            view.fill_(default)
            setattr(b, name, buf.data_ptr())
            out[name] = view.view((n, T) if name == "dead_mask" else (n, T, c))
        for name, dt in _ROW_ARRAYS:
            buf = torch.zeros((m,), dtype=dt, device=dev)
            setattr(b, name, buf.data_ptr())
            out[name] = buf[:n]
        any_alive = torch.zeros((T + 1,), dtype=torch.int32, device=dev)
        b.any_alive = any_alive.data_ptr()
        b.row_slot = self.row_slot.data_ptr() if n else torch.zeros((1,), dtype=torch.int32, device=dev).data_ptr()
        b.n_rows = n
        ms = C.c_float(0.0)
        if time_kernel:
            b.kernel_ms = C.pointer(ms)
        sim.reset(list(range(sim._W)))
        sim._bind_stream()
        _capi.check(sim._L.gd_record_expert(sim._h, C.byref(b), int(n_steps)), "gd_record_expert")
        sim._after()
        self.last_kernel_ms = ms.value if time_kernel else None
        self.any_alive = any_alive
        out.pop("dead")
        return ExpertEpisode(steps=any_alive.sum(), **out)
