"""The device BC update: one gradient step of the reference's imitation learning -- forward, GMM loss, backward, gradient
clipping, AdamW -- as one C call, and the loop over epochs and batches around it.

`DeviceBC` is the body of the reference's training loop (baselines/il/il.py:238-342) for `EarlyFusionAttnBCNet`:
`gd_bc_update` runs `gd_bc_forward` (the deterministic action and the per-row nll of the weights before the step),
`gd_bc_train_rows` (the step's loss and action errors, the upstream gradient of `loss.mean()`), `gd_bc_backward`, and
`clip_grad_norm_(20)`, the reference's `get_grad_norm` and `torch.optim.AdamW` (`gd_bc_adamw`) without a host
synchronisation or an allocation.  The rule -- every rounding, the order of every sum -- is csrc/bc_opt_rule.hpp.

    bc = DeviceBC(net.state_dict(), max_agents=128, num_stack=5, num_layer=(3, 2), num_head=4, head_num_layers=2,
                  n_components=6, clip_value=-20.0, batch_size=512, learning_rate=5e-4)       # il.yaml's values
    bc.fit(ds, total_gradient_steps=1000)     # ds: a DeviceExpertDataset; epochs of shuffled batches, stops in mid-epoch
    bc.losses()                               # one host read: the means over the updates since the last call
    bc.evaluate(eval_ds)                      # bc.policy is a DeviceBCPolicy that follows the optimiser in place
    torch.save(bc.state_dict(), path)         # the reference module's names

Every parameter has exactly one place in the packed weights the forward reads (`gd_bc_policy.blob`), so the AdamW kernel
stores each updated weight to the flat layout and to the blob, and `bc.policy` follows the optimiser with no re-pack.  The
forward of the step runs twice, once for the statistics and once inside the backward's recomputation (about 4 % of a step each),
as it does with `TrainableBCPolicy`, whose autograd forward and backward are the same two calls.

`DeviceBCDim` is the same object at the widths the step is built at, 64 and 128: `network_dim=128` (with head_dim 64 and
num_layer (4, 3): the model of the reference's sweep, baselines/il/sweep.yaml) is `gd_bc_update_dim`, the same four stages
through `gd_bc_forward_dim`, `gd_bc_backward_dim` and `gd_bc_adamw_dim`; the optimiser's kernels have no width in them.

    bc = DeviceBCDim(net.state_dict(), max_agents=128, num_stack=5, num_layer=(4, 3), network_dim=128, partials=32)

`DeviceBC` itself keeps refusing any width but 64, as `gd_bc_update` keeps taking a `gd_bc_policy`.

Not here: the aux head / `use_tom`; `l1_loss` / `focal_loss`; non-zero dropout; bf16; amsgrad; best-checkpoint saving and
wandb logging (the caller's: `evaluate`, `state_dict` and `losses` are what they need); a faster `gd_bc_backward`."""
import ctypes as C
import math

import numpy as np
import torch

from . import _capi
from . import bc_policy as BP
from .bc_train import DEFAULT_PARTIALS, MAX_PARTIALS, grad_floats, grad_scratch_floats

STATS = _capi.BC_STATS
WHO = "DeviceBC: "


def blob_of(num_stack, num_layer, head_num_layers, n_components, *, network_dim=BP.DIM):
    """The inverse of `bc_policy.pack_index` at network_dim: blob_of[e] is the one place of flat parameter e in
    `gd_bc_policy.blob`.  int32 numpy [G].  ValueError if some parameter had no place or more than one (the layout gives every
    parameter exactly one, at either width)."""
    width = {} if network_dim == BP.DIM else dict(network_dim=network_dim)  # (64 is both functions' default)
    index = BP.pack_index(num_stack, num_layer, head_num_layers, n_components, **width)
    G = grad_floats(num_stack, num_layer, head_num_layers, n_components, **width)
    if index.min() < 0 or index.max() > G or (np.bincount(index, minlength=G + 1)[:G] != 1).any():
        raise ValueError("blob_of: a parameter without exactly one place in the blob")
    inv = np.empty(G + 1, dtype=np.int64)
    inv[index] = np.arange(index.size)
    return inv[:G].astype(np.int32)


def tensor_end(shapes):
    """The cumulative element counts of the state dict's tensors: int32 numpy [T]."""
    return np.cumsum([int(np.prod(s)) for s in shapes.values()]).astype(np.int32)


def _number(v):
    return isinstance(v, (int, float)) and not isinstance(v, bool) and math.isfinite(v)


def check_opt_args(batch_size, learning_rate, betas, eps, weight_decay, max_grad_norm, partials, who=WHO):
    """The optimiser's arguments checked on the host (ValueError).  Returns partials."""
    if not BP._is_int(batch_size) or not 1 <= batch_size <= BP.MAX_ROWS:
        raise ValueError(who + "batch_size must be an int in [1, %d], got %r" % (BP.MAX_ROWS, batch_size))
    try:
        b1, b2 = betas
    except (TypeError, ValueError):
        raise ValueError(who + "betas must be a pair of numbers")
    if not (_number(b1) and _number(b2) and 0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
        raise ValueError(who + "betas must lie in [0, 1), got %r" % (betas,))
    for name, v in (("eps", eps), ("max_grad_norm", max_grad_norm), ("learning_rate", learning_rate)):
        if not _number(v) or not v > 0:
            raise ValueError(who + "%s must be a positive number, got %r" % (name, v))
    if not _number(weight_decay) or weight_decay < 0:
        raise ValueError(who + "weight_decay must be a finite number that is not negative, got %r" % (weight_decay,))
    if partials is None:
        partials = DEFAULT_PARTIALS
    if not BP._is_int(partials) or not 1 <= partials <= MAX_PARTIALS:
        raise ValueError(who + "partials must be an int in [1, %d], got %r" % (MAX_PARTIALS, partials))
    return partials


class DeviceBC:
    NETWORK_DIMS = (BP.DIM,)  # the widths this name accepts; `DeviceBCDim` is the class at every width that is built

    def __init__(self, state_dict, max_agents=128, num_stack=5, num_layer=(3, 2), num_head=4, head_num_layers=2,
                 n_components=6, clip_value=-20.0, *, batch_size=512, learning_rate=5e-4, betas=(0.9, 0.999), eps=1e-4,
                 weight_decay=0.01, max_grad_norm=20.0, partials=None, chunk_rows=BP.DEFAULT_CHUNK, device="cuda", **fixed):
        """state_dict and the model arguments: `DeviceBCPolicy`'s (fixed: network_dim, head_dim, network_num_layers, act_func,
        dropout, action_dim, time_dim, use_tom at the values that are built; network_dim must be one of the class's
        NETWORK_DIMS).  batch_size: the most rows an `update` takes.  The hyper-parameters are il.yaml's and il.py:210, 286's:
        `torch.optim.AdamW(lr, betas, eps, weight_decay)` without amsgrad, `clip_grad_norm_(max_grad_norm)`.  partials,
        chunk_rows: `TrainableBCPolicy`'s (None: 128 partial gradients).  Everything is allocated here, once (`nbytes`):
        `partials` times the parameters is the largest part -- 150 MB at the defaults, and 716 MB beside 266 MB of backward
        scratch at the sweep's model (network_dim 128, num_layer (4, 3), 1,399,274 parameters) -- and `partials` is the knob
        where that is too much.  Anything not built is a ValueError raised before anything reaches the device."""
        unknown = sorted(set(fixed) - BP.FIXED)
        if unknown:
            raise ValueError(WHO + "unknown argument(s) %s" % ", ".join(unknown))
        num_layer = tuple(num_layer) if isinstance(num_layer, list) else num_layer
        model = dict(max_agents=max_agents, num_stack=num_stack, num_layer=num_layer, num_head=num_head,
                     head_num_layers=head_num_layers, n_components=n_components, clip_value=clip_value, chunk_rows=chunk_rows,
                     **fixed)
        self._shapes = BP.check_bc_args(state_dict, who=WHO, network_dims=self.NETWORK_DIMS, **model)
        self.network_dim = D = fixed.get("network_dim", BP.DIM)
        self._wide = D != BP.DIM  # a 64-wide instance of either class calls gd_bc_update
        self.partials = check_opt_args(batch_size, learning_rate, betas, eps, weight_decay, max_grad_norm, partials)
        self.policy = BP.DeviceBCPolicy(state_dict, device=device, **model)  # (network_dim travels in `fixed`)
        self.max_agents, self.num_stack, self.num_layer = max_agents, num_stack, num_layer
        self.head_num_layers, self.n_components, self.chunk_rows = head_num_layers, n_components, chunk_rows
        self.batch_size, self.obs_width, self.device = batch_size, self.policy.obs_width, self.policy.device
        self.learning_rate, self.betas, self.eps = float(learning_rate), (float(betas[0]), float(betas[1])), float(eps)
        self.weight_decay, self.max_grad_norm = float(weight_decay), float(max_grad_norm)
        self._names = tuple(self._shapes)
        layout = (num_stack, num_layer, head_num_layers, n_components)
        G = self.G = grad_floats(*layout, network_dim=D)
        T, M, dev, f = len(self._names), batch_size, self.device, torch.float32
        self._own = []

        def new(shape, dtype=f, fill=None):
            t = torch.empty(shape, dtype=dtype, device=dev) if fill is None else torch.full(shape, fill, dtype=dtype, device=dev)
            self._own.append(t)
            return t

        self.flat = new((G + 1,), fill=0.0)  # the weights in the flat layout; the trailing zero stays zero
        with torch.no_grad():
            self.flat[:G].copy_(torch.cat([state_dict[k].detach().to(dev).reshape(-1) for k in self._names]))
        self.exp_avg, self.exp_avg_sq = new((G,), fill=0.0), new((G,), fill=0.0)
        self._blob_of, self._tensor_end = new((G,), torch.int32), new((T,), torch.int32)
        self._blob_of.copy_(torch.from_numpy(blob_of(*layout, network_dim=D)))
        self._tensor_end.copy_(torch.from_numpy(tensor_end(self._shapes)))
        self.grad, self._partials = new((G,)), new((self.partials, G))
        self._grad_scratch = new((grad_scratch_floats(max_agents, chunk_rows, num_layer, self.policy.blob.numel(),
                                                      network_dim=D),))
        self._actions, self._nll, self._grad_nll = new((M, 3)), new((M,)), new((M,))
        self._lr, self._step = new((1,), fill=self.learning_rate), new((1,), torch.int32, fill=0)
        self._beta_pow = new((2,), torch.float64, fill=1.0)
        # what losses() reads, in one buffer: the six running sums and the last update's largest tensor
        self._read = new((7,), torch.int32, fill=0)
        self.stats_sum, self.max_grad_tensor = self._read[:6].view(f), self._read[6:]
        self.stats, self.tensor_norms = new((6,), fill=0.0), new((T,), fill=0.0)
        self._scal = new((4 + 2 * T,), fill=0.0)
        self._updates = 0    # updates since the last losses()
        self._updated = False  # an update was ever made (max_grad_tensor is one's)
        self.host_reads = 0  # reads of the device by losses()
        self._L = _capi.lib()
        # at 128 the gd_bc_policy is the base of the gd_bc_policy_dim that gd_bc_update_dim takes
        self._pd = _capi.GdBCPolicyDim(network_dim=D, reserved=0) if self._wide else None
        p, g, o = self._p, self._g, self._o = self._pd.base if self._wide else _capi.GdBCPolicy(), _capi.GdBCGrad(), _capi.GdBCOpt()
        p.max_agents, p.num_stack, p.fusion_layers, p.branch_layers = max_agents, num_stack, *num_layer
        p.head_layers, p.n_components, p.clip_value, p.chunk_rows = head_num_layers, n_components, float(clip_value), chunk_rows
        p.blob, p.blob_floats = self.policy.blob.data_ptr(), self.policy.blob.numel()
        p.scratch, p.scratch_floats = self.policy._scratch.data_ptr(), self.policy._scratch.numel()
        g.scratch, g.scratch_floats = self._grad_scratch.data_ptr(), self._grad_scratch.numel()
        g.partials, g.grad_floats, g.num_partials = self._partials.data_ptr(), G, self.partials
        o.max_grad_norm, o.eps, o.weight_decay, o.stats_scale = self.max_grad_norm, self.eps, self.weight_decay, 1.0
        o.beta1, o.beta2 = self.betas
        o.grad_floats, o.blob_floats = G, self.policy.blob.numel()
        o.num_stack, o.fusion_layers, o.branch_layers = num_stack, *num_layer
        o.head_layers, o.n_components, o.num_tensors, o.max_rows = head_num_layers, n_components, T, M
        o.tensor_end, o.lr, o.step, o.beta_pow = (t.data_ptr() for t in (self._tensor_end, self._lr, self._step, self._beta_pow))
        o.params, o.exp_avg, o.exp_avg_sq = self.flat.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr()
        o.blob, o.blob_of = self.policy.blob.data_ptr(), self._blob_of.data_ptr()
        o.stats, o.stats_sum, o.max_grad_tensor = self.stats.data_ptr(), self.stats_sum.data_ptr(), self.max_grad_tensor.data_ptr()
        o.tensor_norms, o.scal = self.tensor_norms.data_ptr(), self._scal.data_ptr()
        o.actions, o.nll, o.grad_nll = self._actions.data_ptr(), self._nll.data_ptr(), self._grad_nll.data_ptr()
        o.grad = self.grad.data_ptr()

    @property
    def nbytes(self):
        """Everything the object allocates: the policy's blob, index and forward scratch, the flat weights, both moments, the
        gradient, its partials and the backward's scratch (sized to chunk_rows, not to the batch), the row scratch for
        batch_size rows, the scalars.  At the defaults (partials 128, chunk_rows 128, A = 128) the sweep's model at network_dim
        128 has 716 MB of partial gradients and 266 MB of backward scratch in it."""
        ts = self._own + [self.policy.blob, self.policy._index, self.policy._zero, self.policy._scratch]
        return sum(t.numel() * t.element_size() for t in ts)

    def update(self, obs, expert_actions, partner_mask, road_mask):
        """One gradient step on the tensors `DeviceExpertDataset.batch` writes, in its order: obs [B, R, D] float32,
        expert_actions [B, 1, 3] or [B, 3] float32, partner_mask [B, R, A - 1] and road_mask [B, R, 200] bool or uint8,
        contiguous, on the device, 1 <= B <= batch_size (the short last batch of an epoch is a step like any other).  One C
        call on torch's current stream, no host synchronisation, no allocation.  Afterwards the weights, the moments,
        `policy.blob`, `grad`, `tensor_norms` and `stats` are the step's; nothing is returned."""
        B = self.policy._inputs(obs, partner_mask, road_mask)
        if B > self.batch_size:
            raise ValueError(WHO + "update: B = %d is above batch_size %d" % (B, self.batch_size))
        expert = self.policy._expert(expert_actions, B)
        with torch.cuda.device(self.device):
            stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            entry, who, p = ((self._L.gd_bc_update_dim, "gd_bc_update_dim", self._pd) if self._wide
                             else (self._L.gd_bc_update, "gd_bc_update", self._p))
            _capi.check(entry(C.byref(p), C.byref(self._g), C.byref(self._o), obs.data_ptr(), partner_mask.data_ptr(),
                              road_mask.data_ptr(), B, expert.data_ptr(), stream), who)
        self._updates += 1
        self._updated = True

    def fit(self, ds, total_gradient_steps, generator=None):
        """The reference's outer loop (il.py:238-292): epochs of `ds.batches(batch_size, shuffle=True, generator=generator)`,
        an `update` per batch, until total_gradient_steps updates are made -- in mid-epoch if that is where the count is
        reached.  No host synchronisation beyond what `batches` itself does.  Returns the number of updates made."""
        if not hasattr(ds, "batches") or not hasattr(ds, "__len__"):
            raise ValueError(WHO + "fit: ds must be a DeviceExpertDataset")
        if not BP._is_int(total_gradient_steps) or total_gradient_steps < 0:
            raise ValueError(WHO + "fit: total_gradient_steps must be an int that is not negative, got %r" % (total_gradient_steps,))
        if len(ds) == 0:
            raise ValueError(WHO + "fit: the dataset is empty")
        steps = 0
        while steps < total_gradient_steps:
            for obs, expert, pm, rm, _ in ds.batches(self.batch_size, shuffle=True, generator=generator):
                self.update(obs, expert, pm, rm)
                steps += 1
                if steps >= total_gradient_steps:   # (before the next batch is gathered)
                    break
        return steps

    def losses(self):
        """The means over the updates since the last call of loss, dx_loss, dy_loss, dyaw_loss (il.py:294-306), grad_norm (the
        norm before clipping) and max_grad_norm (the largest tensor norm after clipping, il.py:287) as floats, and
        max_grad_name, the name of the tensor that had it in the LAST update (None before the first): ONE read of the device
        (counted in `host_reads`), after which the sums start again.  Every value is the float32 running sum the kernels
        keep, divided by the number of updates; with no update since the last call, zeros."""
        host = self._read.cpu()
        self.host_reads += 1
        self.stats_sum.zero_()
        n, self._updates = max(self._updates, 1), 0
        out = {k: float(v) / n for k, v in zip(STATS, host[:6].view(torch.float32).tolist())}
        t = int(host[6])
        out["max_grad_name"] = self._names[t] if self._updated and 0 <= t < len(self._names) else None
        return out

    def evaluate(self, ds, batch_size=None):
        """`policy.evaluate`: the reference's evaluate() on the current weights (batch_size None: the training one)."""
        return self.policy.evaluate(ds, self.batch_size if batch_size is None else batch_size)

    def set_learning_rate(self, x):
        """Fill the device scalar the next update reads."""
        if not _number(x) or not x > 0:
            raise ValueError(WHO + "set_learning_rate: a positive number, got %r" % (x,))
        self.learning_rate = float(x)
        self._lr.fill_(self.learning_rate)

    def _views(self, flat):
        o = 0
        for k, shape in self._shapes.items():
            size = int(np.prod(shape))
            yield k, flat[o:o + size].view(shape)
            o += size

    def state_dict(self):
        """The parameters under the reference's names: clones of the flat buffer's views."""
        return {k: v.clone() for k, v in self._views(self.flat)}

    def _group(self):
        probe = torch.optim.AdamW([torch.zeros(1)], lr=self.learning_rate, betas=self.betas, eps=self.eps,
                                  weight_decay=self.weight_decay, amsgrad=False)
        group = dict(probe.state_dict()["param_groups"][0])
        group["params"] = list(range(len(self._names)))
        return group

    def optimizer_state_dict(self):
        """`torch.optim.AdamW.state_dict()`'s format: per parameter, in `expected_shapes` order, `step` (a float32 scalar, as
        torch keeps it), `exp_avg` and `exp_avg_sq`; one param group with this torch's own keys.  It loads into a
        `torch.optim.AdamW` over `TrainableBCPolicy.parameters()`, and that optimiser's loads here.  (One host read: the step
        count.)"""
        step = float(self._step.item())
        state = {}
        for i, ((_, m), (_, v)) in enumerate(zip(self._views(self.exp_avg), self._views(self.exp_avg_sq))):
            state[i] = {"step": torch.tensor(step), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
        return {"state": state, "param_groups": [self._group()]}

    def load_optimizer_state_dict(self, sd):
        """The inverse: moments and step count from a `torch.optim.AdamW` state dict over the same parameters (every
        parameter's `step` must agree; an empty state is a fresh optimiser), and the learning rate and the weight decay of
        its param group.  Its betas and eps must be this object's.  The running products of the betas are rebuilt by `step`
        float64 multiplications, as the kernel builds them."""
        who = WHO + "load_optimizer_state_dict: "
        try:
            state, groups = sd["state"], sd["param_groups"]
        except (TypeError, KeyError):
            raise ValueError(who + "not an optimiser state dict")
        n = len(self._names)
        if len(groups) != 1 or list(groups[0].get("params", ())) != list(range(n)):
            raise ValueError(who + "one param group over the %d parameters is expected" % n)
        group = groups[0]
        if group.get("amsgrad", False) or group.get("maximize", False):
            raise ValueError(who + "amsgrad and maximize are not built")
        if tuple(group.get("betas", self.betas)) != self.betas or group.get("eps", self.eps) != self.eps:
            raise ValueError(who + "betas %r and eps %r are expected" % (self.betas, self.eps))
        wd = group.get("weight_decay", self.weight_decay)
        if not _number(wd) or wd < 0:
            raise ValueError(who + "weight_decay must be a finite number that is not negative, got %r" % (wd,))
        if "lr" in group and (not _number(group["lr"]) or not group["lr"] > 0):
            raise ValueError(who + "lr must be a positive number, got %r" % (group["lr"],))
        if len(state) not in (0, n) or (state and sorted(state) != list(range(n))):
            raise ValueError(who + "state for none or all of the %d parameters is expected" % n)
        try:
            steps = {int(float(state[i]["step"])) for i in state} or {0}
        except (TypeError, KeyError, ValueError):
            raise ValueError(who + "every parameter's state must carry step, exp_avg and exp_avg_sq")
        if len(steps) != 1 or min(steps) < 0:
            raise ValueError(who + "every parameter must carry the same non-negative step")
        for i, shape in enumerate(self._shapes.values()):
            if state and any(not isinstance(state[i].get(k), torch.Tensor) or tuple(state[i][k].shape) != shape
                             or state[i][k].dtype != torch.float32 for k in ("exp_avg", "exp_avg_sq")):
                raise ValueError(who + "parameter %d: float32 moments of shape %s are expected" % (i, shape))
        step = steps.pop()
        for name, mine in (("exp_avg", self.exp_avg), ("exp_avg_sq", self.exp_avg_sq)):
            for i, (_, view) in enumerate(self._views(mine)):
                if state:
                    view.copy_(state[i][name])
                else:
                    view.zero_()
        pw = [1.0, 1.0]
        for _ in range(step):
            pw[0] *= self.betas[0]
            pw[1] *= self.betas[1]
        self._step.fill_(step)
        self._beta_pow.copy_(torch.tensor(pw, dtype=torch.float64))
        self.weight_decay = self._o.weight_decay = float(wd)
        if "lr" in group:
            self.set_learning_rate(group["lr"])


class DeviceBCDim(DeviceBC):
    """`DeviceBC` at every width the step is built at: `network_dim=64` (the default; the same C call and bits as `DeviceBC`)
    or `network_dim=128`, the reference sweep's model, through `gd_bc_update_dim`.  `policy` is a `DeviceBCPolicy` of that width
    and follows the optimiser in place; the optimiser state interchanges with a `torch.optim.AdamW` over
    `TrainableBCPolicyDim.parameters()`.  At 128 the defaults allocate about 1 GB (`nbytes`): pass a smaller `partials`
    where that is too much."""
    NETWORK_DIMS = (BP.DIM, 128)
