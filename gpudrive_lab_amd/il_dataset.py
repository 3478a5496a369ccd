"""The device expert dataset: imitation-learning batches gathered where the recorder wrote the data.

`DeviceExpertDataset` is the reference's `ExpertDataset` (gpudrive/integrations/il/dataloader.py:5-71, 183-211) in its
windowed mode, together with the DataLoader around it (baselines/il/il.py:70-97): the index of valid (row, time) samples is
built on the device (`gd_il_index`, two launches with a prefix sum between them) and `batch()` gathers a training batch with
one kernel (`gd_il_batch`) into the five tensors baselines/il/il.py:248-263 unpacks -- stacked observation windows with their
zero prefix, the action targets, both masks and the sample indices.  The recorded arrays are neither copied nor padded, and
several recorded episodes (shards) train together without being concatenated.

`DeviceFutureDataset` is the third consumer of the same recording: the linear-probing dataset, the reference's `FutureDataset`
(gpudrive/integrations/il/linear_probing/dataloader.py, unpacked by baselines/il/linear_probing.py:173).  Same shards, same
index; `batch()` is one kernel (`gd_il_future_batch`) that returns the window, the targets and the masks together with the
future mask and the 64-class future position labels, which it computes per sample from the recorded ego pose.

Not here: `use_tom` of `ExpertDataset` (the reference cannot run it, dataloader.py:34 against :73) and the flat 2-D mode the
reference falls into when rollout_len + pred_len > 91 (a ValueError here)."""
import ctypes as C
import math

import numpy as np
import torch

from . import _capi
from .recorder import EPISODE_LEN, ROAD_POINTS, packed_width

MAX_SHARDS = _capi.IL_MAX_SHARDS
_FIELDS = ("obs", "actions", "dead_mask", "partner_mask", "road_mask", "keep")
_POSE_FIELDS = ("ego_global_pos", "ego_global_rot")
_AGENTS_OF_WIDTH = {packed_width(A): A for A in (64, 128)}


def _check_window(rollout_len, pred_len):
    ok = all(isinstance(v, int) and not isinstance(v, bool) for v in (rollout_len, pred_len))
    if not ok or rollout_len < 1 or pred_len < 1 or rollout_len + pred_len > EPISODE_LEN:
        raise ValueError("DeviceExpertDataset: rollout_len >= 1, pred_len >= 1 and rollout_len + pred_len <= 91 are required "
                         "(outside it the reference switches to its flat mode), got %r and %r" % (rollout_len, pred_len))


def _check_batch_size(batch_size):
    if not isinstance(batch_size, int) or isinstance(batch_size, bool) or batch_size < 1:
        raise ValueError("DeviceExpertDataset.batches: batch_size must be a positive int, got %r" % (batch_size,))


def _check_shard(i, ep, who="DeviceExpertDataset", pose=False):
    """One shard's six tensors (and the two of the ego pose, if asked for), checked without touching them; returns
    (tensors, N, A)."""
    get = (lambda k: ep.get(k)) if isinstance(ep, dict) else (lambda k: getattr(ep, k, None))
    t = {k: get(k) for k in _FIELDS + (_POSE_FIELDS if pose else ())}
    what = "%s: shard %d " % (who, i)
    for k, v in t.items():
        if not isinstance(v, torch.Tensor):
            raise ValueError(what + "%s must be a tensor, got %s" % (k, type(v).__name__))
    want = dict(obs=torch.float32, actions=torch.float32, dead_mask=torch.bool, partner_mask=torch.uint8,
                road_mask=torch.bool, keep=torch.bool)
    if pose:
        want.update(ego_global_pos=torch.float32, ego_global_rot=torch.float32)
    for k, dt in want.items():
        if t[k].dtype != dt:
            raise ValueError(what + "%s must be %s, got %s" % (k, dt, t[k].dtype))
    obs = t["obs"]
    if obs.dim() != 3 or obs.shape[1] != EPISODE_LEN or obs.shape[2] not in _AGENTS_OF_WIDTH:
        raise ValueError(what + "obs must be [N, 91, D] with D = 2984 (64 agent slots) or 3368 (128), got %s" % (tuple(obs.shape),))
    N, A = int(obs.shape[0]), _AGENTS_OF_WIDTH[int(obs.shape[2])]
    shapes = dict(actions=(N, EPISODE_LEN, 3), dead_mask=(N, EPISODE_LEN), partner_mask=(N, EPISODE_LEN, A - 1),
                  road_mask=(N, EPISODE_LEN, ROAD_POINTS), keep=(N,))
    if pose:
        shapes.update(ego_global_pos=(N, EPISODE_LEN, 2), ego_global_rot=(N, EPISODE_LEN, 1))
    for k, shp in shapes.items():
        if tuple(t[k].shape) != shp:
            raise ValueError(what + "%s must be %s beside obs %s, got %s" % (k, shp, tuple(obs.shape), tuple(t[k].shape)))
    for k, v in t.items():
        if v.device != obs.device:
            raise ValueError(what + "%s is on %s, obs on %s" % (k, v.device, obs.device))
        if not v.is_contiguous():
            raise ValueError(what + "%s must be contiguous" % k)
    return t, N, A


class DeviceExpertDataset:
    _POSE = False  # whether a shard must carry the ego pose as well (DeviceFutureDataset)

    def __init__(self, episodes, rollout_len=5, pred_len=1):
        """episodes: one `ExpertEpisode`, or a dict of the same device tensors (obs, actions, dead_mask, partner_mask,
        road_mask, keep), or a list of up to 8 of either: the shards, in the order the reference would concatenate their files
        (data_concat.py).  Every argument is checked before anything reaches the device (ValueError).  One host
        synchronisation, here, for the number of samples."""
        _check_window(rollout_len, pred_len)
        if not isinstance(episodes, (list, tuple)):
            episodes = [episodes]
        if len(episodes) > MAX_SHARDS:
            raise ValueError("DeviceExpertDataset: at most %d shards, got %d" % (MAX_SHARDS, len(episodes)))
        if not episodes:
            raise ValueError("DeviceExpertDataset: no episode given")
        shards = [_check_shard(i, ep, type(self).__name__, self._POSE) for i, ep in enumerate(episodes)]
        agents = {A for _, _, A in shards}
        if len(agents) != 1:
            raise ValueError("DeviceExpertDataset: the shards' observation widths give different agent slot counts: %s"
                             % sorted(agents))
        devices = {t["obs"].device for t, _, _ in shards}
        if len(devices) != 1:
            raise ValueError("DeviceExpertDataset: the shards are on different devices: %s" % sorted(map(str, devices)))
        self.device = devices.pop()
        if self.device.type != "cuda":
            raise ValueError("DeviceExpertDataset: the tensors must be on the GPU (there is no host path), got %s" % self.device)
        for i, (t, N, _) in enumerate(shards):
            if N and (t["obs"].data_ptr() % 16 or t["road_mask"].data_ptr() % 8):
                raise ValueError("DeviceExpertDataset: shard %d: obs must be 16-byte aligned and road_mask 8-byte aligned" % i)
        self.rollout_len, self.pred_len, self.max_agents = rollout_len, pred_len, agents.pop()
        self.obs_width = packed_width(self.max_agents)
        self._shards = [t for t, N, _ in shards if N]  # (kept alive; a shard without rows has nothing to point at)
        self.num_rows = sum(N for _, N, _ in shards)
        d = self._ds = _capi.GdIlDataset()
        d.n_shards, d.max_agents, d.rollout_len, d.pred_len = len(self._shards), self.max_agents, rollout_len, pred_len
        for sh, t in zip(d.shard, self._shards):
            for k in _FIELDS:
                setattr(sh, k, t[k].data_ptr())
            sh.n_rows = int(t["obs"].shape[0])
        self._L = _capi.lib()
        self._build_index()

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _build_index(self):
        dev, rows = self.device, self.num_rows
        self.bad_indices = torch.zeros((1,), dtype=torch.int32, device=dev)
        self._len = 0
        if rows:
            with torch.cuda.device(dev):
                counts = torch.empty((rows,), dtype=torch.int32, device=dev)
                kept = torch.empty((rows,), dtype=torch.int32, device=dev)
                _capi.check(self._L.gd_il_index(C.byref(self._ds), counts.data_ptr(), kept.data_ptr(), None, None, None,
                                                self._stream()), "gd_il_index")
                ends = torch.cumsum(counts, 0, dtype=torch.int64)
                offsets = (ends - counts).contiguous()
                ordinals = (torch.cumsum(kept, 0, dtype=torch.int64) - kept).contiguous()
                self._len = int(ends[-1].item())  # the one host synchronisation
        self._entries = torch.empty((max(self._len, 1), 4), dtype=torch.int32, device=dev)  # {shard, row, idx2, idx1}
        if self._len:
            with torch.cuda.device(dev):
                _capi.check(self._L.gd_il_index(C.byref(self._ds), None, None, offsets.data_ptr(), ordinals.data_ptr(),
                                                self._entries.data_ptr(), self._stream()), "gd_il_index")

    def __len__(self):
        return self._len

    @property
    def valid_indices(self):
        """[M, 2] int64 (idx1, idx2) in the reference's order (dataloader.py:66-71)."""
        return self._entries[:self._len, [3, 2]].to(torch.int64)

    @property
    def nbytes(self):
        """The index and the counter: what the dataset allocates.  The recorded arrays are used in place."""
        return self._entries.numel() * 4 + self.bad_indices.numel() * 4

    def batch_shapes(self, batch):
        """(shape, dtype) of the five outputs of `batch()` for `batch` samples."""
        R, P, A = self.rollout_len, self.pred_len, self.max_agents
        return (((batch, R, self.obs_width), torch.float32), ((batch, P, 3), torch.float32), ((batch, R, A - 1), torch.bool),
                ((batch, R, ROAD_POINTS), torch.bool), ((batch, 2), torch.int64))

    _OUT_NAMES = ("obs", "actions", "partner_mask", "road_mask", "data_idx")
    _OUT_ALIGNED = ((0, 16), (3, 8))  # (output, bytes): what the kernel's wide stores need
    _OUT_ALIGNED_TEXT = "out obs must be 16-byte aligned and road_mask 8-byte aligned"

    def _outputs(self, sel, out):
        """sel and the out= tensors of `batch()` checked; returns (B, the outputs, allocated unless given)."""
        who = type(self).__name__
        if not isinstance(sel, torch.Tensor) or sel.dtype != torch.int64 or sel.dim() != 1 or sel.device != self.device \
                or not sel.is_contiguous():
            raise ValueError("%s.batch: sel must be a contiguous [B] int64 tensor on %s" % (who, self.device))
        B = int(sel.shape[0])
        want = self.batch_shapes(B)
        if out is None:
            return B, tuple(torch.empty(shape, dtype=dt, device=self.device) for shape, dt in want)
        if not isinstance(out, (tuple, list)) or len(out) != len(want):
            raise ValueError("%s.batch: out must be the %s tensors of a batch" % (who, {5: "five", 8: "eight"}[len(want)]))
        for name, o, (shape, dt) in zip(self._OUT_NAMES, out, want):
            if not isinstance(o, torch.Tensor) or o.dtype != dt or o.device != self.device or tuple(o.shape) != shape \
                    or not o.is_contiguous():
                raise ValueError("%s.batch: out %s must be a contiguous %s %s tensor on %s" % (who, name, dt, shape, self.device))
        if B and any(out[i].data_ptr() % n for i, n in self._OUT_ALIGNED):
            raise ValueError("%s.batch: %s" % (who, self._OUT_ALIGNED_TEXT))
        return B, tuple(out)

    def batch(self, sel, out=None):
        """Gather the samples at positions `sel` ([B] int64 on the device; any order, repeats allowed) of the index:
        (obs [B, R, D] f32, actions [B, P, 3] f32, partner_mask [B, R, A - 1] bool, road_mask [B, R, 200] bool,
        data_idx [B, 2] int64), what baselines/il/il.py:248-263 unpacks.  One launch on torch's current stream, no host
        synchronisation.  A position outside [0, len) gives an all-padding sample (obs 0, actions 0, masks True, data_idx
        (-1, -1)) and counts in `bad_indices`.  out: the five tensors of an earlier call with the same B, to be overwritten."""
        B, out = self._outputs(sel, out)
        if B == 0:
            return out
        b = _capi.GdIlBatchBuffers()
        b.entries, b.n_entries, b.sel, b.batch = self._entries.data_ptr(), self._len, sel.data_ptr(), B
        b.bad_indices = self.bad_indices.data_ptr()
        b.obs, b.actions, b.partner_mask, b.road_mask, b.data_idx = (o.data_ptr() for o in out)
        with torch.cuda.device(self.device):
            _capi.check(self._L.gd_il_batch(C.byref(self._ds), C.byref(b), self._stream()), "gd_il_batch")
        return out

    @staticmethod
    def batch_selections(order, batch_size, drop_last=False):
        """The slices of `order` (a permutation of the sample positions) one epoch's batches take: consecutive runs of
        batch_size, the last one short unless drop_last drops it (torch's DataLoader, il.py:88-95)."""
        _check_batch_size(batch_size)
        n = int(order.shape[0])
        end = n - n % batch_size if drop_last else n
        for lo in range(0, end, batch_size):
            yield order[lo:min(lo + batch_size, end)]

    def batches(self, batch_size, shuffle=True, generator=None, drop_last=False):
        """One epoch: yields `batch()` of consecutive runs of a permutation drawn on the device (`torch.randperm` with
        `generator`, a device generator; the identity without shuffle)."""
        _check_batch_size(batch_size)
        if shuffle:
            order = torch.randperm(self._len, device=self.device, generator=generator)
        else:
            order = torch.arange(self._len, device=self.device)
        for sel in self.batch_selections(order, batch_size, drop_last):
            yield self.batch(sel)


def _check_future(future_step, exp, xy_range):
    """The arguments of DeviceFutureDataset that are its own; returns (exp code, xbins, ybins)."""
    if not isinstance(future_step, int) or isinstance(future_step, bool) or not 1 <= future_step <= EPISODE_LEN - 1:
        raise ValueError("DeviceFutureDataset: future_step must be an int in [1, 90], got %r" % (future_step,))
    if exp not in ("other", "ego"):
        raise ValueError("DeviceFutureDataset: exp must be 'other' or 'ego', got %r" % (exp,))
    ranges = ((-0.05, 0.05), (-0.05, 0.05))  # dataloader.py:161-162
    if xy_range is not None:
        if exp == "other":
            raise ValueError("DeviceFutureDataset: xy_range is for exp='ego' only (the reference ignores it for 'other', "
                             "dataloader.py:53)")
        try:
            ranges = tuple((float(lo), float(hi)) for lo, hi in xy_range)
        except (TypeError, ValueError):
            ranges = ()
        if len(ranges) != 2 or not all(math.isfinite(lo) and math.isfinite(hi) and lo < hi for lo, hi in ranges):
            raise ValueError("DeviceFutureDataset: xy_range must be ((xlo, xhi), (ylo, yhi)), finite with lo < hi, got %r"
                             % (xy_range,))
    bins = [np.linspace(lo, hi, 9) for lo, hi in ranges]
    for b in bins:
        if not (np.isfinite(b).all() and (np.diff(b) > 0).all()):
            raise ValueError("DeviceFutureDataset: xy_range %r gives bin edges that do not increase" % (xy_range,))
    return (_capi.IL_FUTURE_OTHER if exp == "other" else _capi.IL_FUTURE_EGO), bins[0], bins[1]


class DeviceFutureDataset(DeviceExpertDataset):
    _POSE = True
    OUT_NAMES = {"other": ("obs", "actions", "valid_mask", "ego_mask", "partner_mask", "road_mask", "aux_mask", "other_pos"),
                 "ego": ("obs", "actions", "valid_mask", "ego_mask", "partner_mask", "road_mask", "future_valid_mask", "ego_pos")}
    _OUT_ALIGNED = ((0, 16), (5, 8), (7, 8))
    _OUT_ALIGNED_TEXT = "out obs must be 16-byte aligned, road_mask and the labels 8-byte aligned"

    def __init__(self, episodes, rollout_len=5, pred_len=1, future_step=1, exp="other", xy_range=None):
        """episodes: as `DeviceExpertDataset`, every shard with `ego_global_pos` [N, 91, 2] and `ego_global_rot` [N, 91, 1]
        (f32, contiguous) as well.  future_step: 1..90.  exp: 'other' (the partners' positions future_step ahead, in the
        ego's current frame) or 'ego' (the ego's own displacement).  xy_range: ((xlo, xhi), (ylo, yhi)) of the 8 x 8 classes,
        'ego' only; (-0.05, 0.05) for both without it.  The index is `DeviceExpertDataset`'s."""
        code, xbins, ybins = _check_future(future_step, exp, xy_range)
        self.future_step, self.exp, self.xbins, self.ybins = future_step, exp, xbins, ybins
        self._OUT_NAMES = self.OUT_NAMES[exp]
        super().__init__(episodes, rollout_len=rollout_len, pred_len=pred_len)
        f = self._future = _capi.GdIlFuture()
        f.future_step, f.exp = future_step, code
        f.xbins[:], f.ybins[:] = xbins.tolist(), ybins.tolist()
        for i, t in enumerate(self._shards):
            f.ego_global_pos[i], f.ego_global_rot[i] = t["ego_global_pos"].data_ptr(), t["ego_global_rot"].data_ptr()

    def batch_shapes(self, batch):
        """(shape, dtype) of the eight outputs of `batch()` for `batch` samples."""
        R, P, A = self.rollout_len, self.pred_len, self.max_agents
        future = (batch, A - 1) if self.exp == "other" else (batch,)
        return (((batch, R, self.obs_width), torch.float32), ((batch, P, 3), torch.float32), ((batch,), torch.bool),
                ((batch, R), torch.bool), ((batch, R, A - 1), torch.bool), ((batch, R, ROAD_POINTS), torch.bool),
                (future, torch.bool), (future, torch.int64))

    def batch(self, sel, out=None):
        """The samples at positions `sel` of the index as the eight tensors baselines/il/linear_probing.py:173 unpacks:
        (obs [B, R, D] f32, actions [B, P, 3] f32, valid_mask [B] bool, ego_mask [B, R] bool, partner_mask [B, R, A - 1] bool,
        road_mask [B, R, 200] bool, then for exp='other' aux_mask [B, A - 1] bool and other_pos [B, A - 1] int64, for exp='ego'
        future_valid_mask [B] bool and ego_pos [B] int64).  obs, actions, partner_mask and road_mask are what
        `DeviceExpertDataset.batch(sel)` gives.  One launch on torch's current stream, no host synchronisation.  A position
        outside [0, len) gives that padding, False in valid_mask, ego_mask and future_valid_mask, True in aux_mask and the
        class of (0, 0) as label, and counts in `bad_indices`.  out: the eight tensors of an earlier call with the same B."""
        B, out = self._outputs(sel, out)
        if B == 0:
            return out
        b = _capi.GdIlFutureBuffers()
        b.entries, b.n_entries, b.sel, b.batch = self._entries.data_ptr(), self._len, sel.data_ptr(), B
        b.bad_indices = self.bad_indices.data_ptr()
        (b.obs, b.actions, b.valid_mask, b.ego_mask, b.partner_mask, b.road_mask, b.future_mask,
         b.future_pos) = (o.data_ptr() for o in out)
        with torch.cuda.device(self.device):
            _capi.check(self._L.gd_il_future_batch(C.byref(self._ds), C.byref(self._future), C.byref(b), self._stream()),
                        "gd_il_future_batch")
        return out
