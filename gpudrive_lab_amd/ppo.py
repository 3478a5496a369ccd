"""The device PPO update: one minibatch of the reference's training loop -- forward for the stored actions, loss, backward,
gradient clipping, Adam -- as one C call, and the loop over epochs and minibatches around it.

`DevicePPO` is the body of the reference's `train` (gpudrive/integrations/puffer/ppo.py:249-342) for the late-fusion
actor-critic: `gd_ppo_update` runs `gd_policy_evaluate`, the loss with its three upstream gradients (`gd_ppo_loss`),
`gd_policy_backward`, and `clip_grad_norm_` plus `torch.optim.Adam` (`gd_ppo_adam`) as nine launches without a host
synchronisation or an allocation.  The rule -- every rounding, the order of every sum -- is csrc/ppo_rule.hpp.

    ppo = DevicePPO(net.state_dict(), max_agents=128, ego_width=6, minibatch_size=8192)   # the puffer yaml's defaults
    pol = ppo.policy                      # a DevicePolicy for the rollout; the optimiser step stores into pol.blob in place
    ... fill ro (a DeviceRollout) with pol ...
    ro.sort_training_data(); ro.compute_gae(gamma, gae_lambda)
    ppo.train(ro, update_epochs=4)
    ppo.losses()                          # one host read: the means over the updates since the last call

Every parameter has exactly one place in the packed weights the forward reads (`gd_policy.blob`), so the Adam kernel stores
each updated weight to the flat layout and to the blob, and `ppo.policy` follows the optimiser with no re-pack.

Training-mode dropout (the yaml's `network.dropout: 0.01`, live in the reference's rollout and update alike) is
`dropout_rule=DropoutRule(p, seed)` (dropout.py): the update's evaluate and backward mask the four sites by the rule, and
`ppo.policy` is handed the same rule, so the rollout and the updates draw from one stream of call indices.

Not here: `target_kl` (it needs a host read per epoch; the yaml's is null), torch's own dropout stream (the numeric
`dropout` stays 0.0), the explained variance (the reference computes it from `returns_np`, which rollout.py documents as a
quirk), LSTM state, weight decay, amsgrad, a bf16 path."""
import ctypes as C
import math

import numpy as np
import torch

from . import _capi
from .dropout import check_rule
from .policy import (DEFAULT_PARTIALS, FEATURES, INPUT_DIM, MAX_PARTIALS, MAX_ROWS, ROWSTAT, DevicePolicy, _is_int,
                     check_policy_args, expected_shapes, grad_floats, pack_index)

STATS = _capi.PPO_STATS


def blob_of(ego_width, n_actions):
    """The inverse of `pack_index`: blob_of[e] is the one place of flat parameter e in `gd_policy.blob`.  int32 numpy [G].
    ValueError if some parameter had no place or more than one (the layout gives every parameter exactly one)."""
    index = pack_index(ego_width, n_actions)
    G = grad_floats(ego_width, n_actions)
    if (np.bincount(index, minlength=G + 1)[:G] != 1).any():
        raise ValueError("blob_of: a parameter without exactly one place in the blob")
    inv = np.empty(G + 1, dtype=np.int64)
    inv[index] = np.arange(index.size)
    return inv[:G].astype(np.int32)


def _number(v):
    return isinstance(v, (int, float)) and not isinstance(v, bool) and math.isfinite(v)


def check_ppo_args(state_dict, max_agents, ego_width, minibatch_size, learning_rate, betas, eps, clip_coef, clip_vloss,
                   vf_clip_coef, norm_adv, ent_coef, vf_coef, max_grad_norm, target_kl, partials, dropout=0.0, act_func="tanh",
                   vbd_in_obs=False, dropout_rule=None):
    """Everything `DevicePPO` refuses, checked on the host before anything reaches the device (ValueError).  Returns
    (n_actions, partials)."""
    who = "DevicePPO: "
    n_actions = check_policy_args(state_dict, max_agents, ego_width, act_func, vbd_in_obs, who=who)
    if target_kl is not None:
        raise ValueError(who + "target_kl is not built (it needs a host read per epoch); pass None")
    if isinstance(dropout, bool) or not isinstance(dropout, (int, float)) or dropout != 0.0:
        raise ValueError(who + "dropout must be 0.0 (nn.Dropout's random stream cannot be reproduced; pass "
                         "dropout_rule=DropoutRule(p, seed) for training-mode masks), got %r" % (dropout,))
    check_rule(dropout_rule, who)
    if not _is_int(minibatch_size) or not 1 <= minibatch_size <= MAX_ROWS:
        raise ValueError(who + "minibatch_size must be an int in [1, %d], got %r" % (MAX_ROWS, minibatch_size))
    if norm_adv and minibatch_size < 2:
        raise ValueError(who + "norm_adv needs minibatch_size >= 2 (the unbiased variance of one advantage is undefined)")
    try:
        b1, b2 = betas
    except (TypeError, ValueError):
        raise ValueError(who + "betas must be a pair of numbers")
    if not (_number(b1) and _number(b2) and 0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
        raise ValueError(who + "betas must lie in [0, 1), got %r" % (betas,))
    for name, v in (("eps", eps), ("max_grad_norm", max_grad_norm), ("learning_rate", learning_rate)):
        if not _number(v) or not v > 0:
            raise ValueError(who + "%s must be a positive number, got %r" % (name, v))
    for name, v in (("clip_coef", clip_coef), ("vf_clip_coef", vf_clip_coef), ("ent_coef", ent_coef), ("vf_coef", vf_coef)):
        if not _number(v):
            raise ValueError(who + "%s must be a finite number, got %r" % (name, v))
    if partials is None:
        partials = DEFAULT_PARTIALS
    if not _is_int(partials) or not 1 <= partials <= MAX_PARTIALS:
        raise ValueError(who + "partials must be an int in [1, %d], got %r" % (MAX_PARTIALS, partials))
    return n_actions, partials


UPDATE_NAMES = ("obs", "actions", "logprobs", "values", "advantages", "returns")


def check_update_args(minibatch_size, obs_width, device, *args):
    """The six arguments of `DevicePPO.update` checked on the host (ValueError): each a contiguous tensor on `device`, obs
    [rows, bptt, obs_width] or [M, obs_width] float32, actions int64 and the four others float32 of shape [rows, bptt] or [M],
    with rows * bptt = M = minibatch_size.  Returns their device pointers."""
    M, f = minibatch_size, torch.float32
    if len(args) != 6:
        raise ValueError("DevicePPO.update: the six tensors %s are expected" % (UPDATE_NAMES,))
    obs = args[0]
    lead = [(M,)]
    if isinstance(obs, torch.Tensor) and obs.dim() == 3 and obs.shape[0] * obs.shape[1] == M:
        lead.append(tuple(obs.shape[:2]))
    ptrs = []
    for name, t in zip(UPDATE_NAMES, args):
        dtype = torch.int64 if name == "actions" else f
        shapes = [s + (obs_width,) for s in lead] if name == "obs" else lead
        if not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) not in shapes or t.device != device \
                or not t.is_contiguous():
            raise ValueError("DevicePPO.update: %s must be a contiguous %s tensor of shape %s on %s"
                             % (name, dtype, " or ".join(map(str, shapes)), device))
        ptrs.append(t.data_ptr())
    return ptrs


def check_train_args(ro, minibatch_size, obs_width, device, update_epochs):
    """What `DevicePPO.train` refuses (ValueError): a rollout of another minibatch size, observation width or device, or with
    more than one action index per entry."""
    from .rollout import DeviceRollout
    who = "DevicePPO.train: "
    if not isinstance(ro, DeviceRollout):
        raise ValueError(who + "ro must be a DeviceRollout")
    if ro.minibatch_size != minibatch_size or ro.obs_width != obs_width or ro.device != device or ro.action_shape != ():
        raise ValueError(who + "the rollout must have minibatch_size %d, obs_width %d, one action index per entry and live on %s"
                         % (minibatch_size, obs_width, device))
    if not _is_int(update_epochs) or update_epochs < 1:
        raise ValueError(who + "update_epochs must be a positive int, got %r" % (update_epochs,))


class DevicePPO:
    def __init__(self, state_dict, max_agents=128, ego_width=6, minibatch_size=8192, *, learning_rate=3e-4, betas=(0.9, 0.999),
                 eps=1e-5, clip_coef=0.2, clip_vloss=False, vf_clip_coef=0.2, norm_adv=True, ent_coef=1e-4, vf_coef=0.3,
                 max_grad_norm=0.5, target_kl=None, partials=None, device="cuda", dropout=0.0, act_func="tanh",
                 vbd_in_obs=False, dropout_rule=None):
        """state_dict, max_agents, ego_width: `DevicePolicy`'s.  minibatch_size: M, the rows of every `update`.  The
        hyper-parameters carry the reference config's names and the puffer yaml's defaults; Adam is `torch.optim.Adam(lr,
        betas, eps)` without weight decay or amsgrad.  partials: `TrainablePolicy`'s (None: 256).  Everything is allocated
        here, once (`nbytes`), except the minibatch buffers of `train`, which its first call adds.  Anything not built is a
        ValueError raised before anything reaches the device.
        dropout_rule: None, or a `DropoutRule` on the same device: every `update` then masks its forward and backward by the
        rule, and `policy` is handed the same rule, so the rollout forwards and the updates consume ONE stream of call indices
        in the order they are enqueued -- they share a CUDA stream (torch's current one), or the caller orders them by events.
        The rule's counter is the rule's own allocation; nothing is allocated per update."""
        self.n_actions, self.partials = check_ppo_args(state_dict, max_agents, ego_width, minibatch_size, learning_rate, betas,
                                                       eps, clip_coef, clip_vloss, vf_clip_coef, norm_adv, ent_coef, vf_coef,
                                                       max_grad_norm, target_kl, partials, dropout, act_func, vbd_in_obs,
                                                       dropout_rule)
        self.policy = DevicePolicy(state_dict, max_agents, ego_width, device=device, dropout_rule=dropout_rule)
        self.dropout_rule = dropout_rule
        self.max_agents, self.ego_width, self.minibatch_size = max_agents, ego_width, minibatch_size
        self.obs_width, self.device = self.policy.obs_width, self.policy.device
        self.learning_rate, self.betas, self.eps = float(learning_rate), (float(betas[0]), float(betas[1])), float(eps)
        self.clip_coef, self.clip_vloss, self.vf_clip_coef = float(clip_coef), bool(clip_vloss), float(vf_clip_coef)
        self.norm_adv, self.ent_coef, self.vf_coef = bool(norm_adv), float(ent_coef), float(vf_coef)
        self.max_grad_norm = float(max_grad_norm)
        self._shapes = expected_shapes(ego_width, self.n_actions)
        G = self.G = grad_floats(ego_width, self.n_actions)
        M, na, dev, f = minibatch_size, self.n_actions, self.device, torch.float32
        self._own = []

        def new(shape, dtype=f, fill=None):
            t = torch.empty(shape, dtype=dtype, device=dev) if fill is None else torch.full(shape, fill, dtype=dtype, device=dev)
            self._own.append(t)
            return t

        self.flat = new((G + 1,), fill=0.0)  # the weights in the flat layout; the trailing zero stays zero
        with torch.no_grad():
            self.flat[:G].copy_(torch.cat([state_dict[k].detach().to(dev).reshape(-1) for k in self._shapes]))
        self.exp_avg, self.exp_avg_sq = new((G,), fill=0.0), new((G,), fill=0.0)
        self._blob_of = new((G,), torch.int32)
        self._blob_of.copy_(torch.from_numpy(blob_of(ego_width, na)))
        self.grad, self._partials = new((G,)), new((self.partials, G))
        self._features, self._logits = new((M, FEATURES)), new((M, na))
        self.winners, self._rowstat = new((M, 2 * INPUT_DIM), torch.uint8), new((M, ROWSTAT))
        self._rows = [new((M,)) for _ in range(6)]  # newlogprob, entropy, newvalue, d_logprob, d_entropy, d_value
        self._lr, self._step = new((1,), fill=self.learning_rate), new((1,), torch.int32, fill=0)
        self._beta_pow = new((2,), torch.float64, fill=1.0)
        self.stats, self.stats_sum, self._scal = new((7,), fill=0.0), new((7,), fill=0.0), new((4,), fill=0.0)
        self._updates = 0   # updates since the last losses()
        self.host_reads = 0  # reads of the device by losses()
        self._mb = None
        self._L = _capi.lib()
        p, g, o = self._p, self._g, self._o = _capi.GdPolicy(), _capi.GdPolicyGrad(), _capi.GdPPO()
        p.num_rows, p.max_agents, p.ego_width, p.n_actions = M, max_agents, ego_width, na
        p.blob, p.blob_floats = self.policy.blob.data_ptr(), self.policy.blob.numel()
        g.features, g.logits, g.winners = self._features.data_ptr(), self._logits.data_ptr(), self.winners.data_ptr()
        g.params, g.rowstat, g.partials = self.flat.data_ptr(), self._rowstat.data_ptr(), self._partials.data_ptr()
        g.grad_floats, g.num_partials = G, self.partials
        o.num_rows, o.ego_width, o.n_actions = M, ego_width, na
        o.norm_adv, o.clip_vloss = int(self.norm_adv), int(self.clip_vloss)
        o.clip_coef, o.vf_clip_coef, o.ent_coef, o.vf_coef = self.clip_coef, self.vf_clip_coef, self.ent_coef, self.vf_coef
        o.max_grad_norm, o.eps, o.stats_scale = self.max_grad_norm, self.eps, 1.0
        o.beta1, o.beta2 = self.betas
        o.grad_floats, o.blob_floats = G, self.policy.blob.numel()
        o.lr, o.step, o.beta_pow = self._lr.data_ptr(), self._step.data_ptr(), self._beta_pow.data_ptr()
        o.params, o.exp_avg, o.exp_avg_sq = self.flat.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr()
        o.blob, o.blob_of = self.policy.blob.data_ptr(), self._blob_of.data_ptr()
        o.stats, o.stats_sum, o.scal = self.stats.data_ptr(), self.stats_sum.data_ptr(), self._scal.data_ptr()
        (o.newlogprob, o.entropy, o.newvalue, o.d_logprob, o.d_entropy, o.d_value) = (t.data_ptr() for t in self._rows)
        o.grad = self.grad.data_ptr()
        # the index an update's evaluate consumes, for its own backward
        self._used = None if dropout_rule is None else new((1,), torch.int64, fill=0)
        self._d = None if dropout_rule is None else dropout_rule.struct(self._used)

    @property
    def nbytes(self):
        """Everything the object allocates: the policy's blob and index, the flat weights, both moments, the gradient and
        its partials, the row scratch for minibatch_size rows, the scalars, and (after the first `train`) one minibatch."""
        ts = self._own + [self.policy.blob, self.policy._index, self.policy._zero] + list(self._mb or ())
        return sum(t.numel() * t.element_size() for t in ts)

    def update(self, obs, actions, logprobs, values, advantages, returns):
        """One minibatch update on the tensors `DeviceRollout.minibatch` returns (its `dones` is not used): obs
        [rows, bptt, obs_width] or [M, obs_width] float32, actions [rows, bptt] or [M] int64, the stored logprobs and values,
        the advantages and the returns [rows, bptt] or [M] float32, M = rows * bptt = minibatch_size, contiguous, on the
        device.  Nine launches on torch's current stream, no host synchronisation, no allocation; with a dropout rule the
        update consumes one call index.  Afterwards the weights,
        the moments, `policy.blob`, `grad`, `winners` and `stats` are the update's; nothing is returned."""
        ptrs = check_update_args(self.minibatch_size, self.obs_width, self.device, obs, actions, logprobs, values, advantages,
                                 returns)
        with torch.cuda.device(self.device):
            stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            if self._d is None:
                _capi.check(self._L.gd_ppo_update(C.byref(self._p), C.byref(self._g), C.byref(self._o), *ptrs, stream),
                            "gd_ppo_update")
            else:
                _capi.check(self._L.gd_ppo_update_dropout(C.byref(self._p), C.byref(self._g), C.byref(self._o), C.byref(self._d),
                                                          *ptrs, stream), "gd_ppo_update_dropout")
        self._updates += 1

    def train(self, ro, update_epochs=4):
        """The reference's loop (ppo.py:249-342) over a sorted `DeviceRollout` with advantages: for every epoch and every
        minibatch in order, `ro.minibatch(mb, out=...)` into the object's own buffers (allocated by the first call) and
        `update`.  No host synchronisation."""
        check_train_args(ro, self.minibatch_size, self.obs_width, self.device, update_epochs)
        want = ro.batch_shapes()
        if self._mb is None or tuple((tuple(t.shape), t.dtype) for t in self._mb) != want:
            self._mb = tuple(torch.empty(shape, dtype=dt, device=self.device) for shape, dt in want)
        for _ in range(update_epochs):
            for mb in range(ro.num_minibatches):
                obs, actions, logprobs, _, values, advantages, returns = ro.minibatch(mb, out=self._mb)
                self.update(obs, actions, logprobs, values, advantages, returns)

    def losses(self):
        """The means over the updates since the last call of policy_loss, value_loss, entropy, old_approx_kl, approx_kl,
        clipfrac (the reference's `losses`) and grad_norm (the norm before clipping), as a dict of floats: ONE read of the
        device (counted in `host_reads`), after which the sums start again.  Every value is the float32 running sum the
        kernels keep, divided by the number of updates; with no update since the last call, zeros."""
        host = self.stats_sum.cpu()
        self.host_reads += 1
        self.stats_sum.zero_()
        n, self._updates = max(self._updates, 1), 0
        return {k: float(v) / n for k, v in zip(STATS, host.tolist())}

    def set_learning_rate(self, x):
        """Fill the device scalar the next update reads (the reference's `anneal_lr`)."""
        if not _number(x) or not x > 0:
            raise ValueError("DevicePPO.set_learning_rate: a positive number, got %r" % (x,))
        self.learning_rate = float(x)
        self._lr.fill_(self.learning_rate)

    def state_dict(self):
        """The parameters under the reference's names: clones of the flat buffer's views."""
        out, o = {}, 0
        for k, shape in self._shapes.items():
            size = int(np.prod(shape))
            out[k] = self.flat[o:o + size].view(shape).clone()
            o += size
        return out

    def optimizer_state_dict(self):
        """`torch.optim.Adam.state_dict()`'s format: per parameter, in `expected_shapes` order, `step` (a float32 scalar, as
        torch keeps it), `exp_avg` and `exp_avg_sq`; one param group.  It loads into the reference's optimiser over the same
        module, and the reference's loads here.  (One host read: the step count.)"""
        step = float(self._step.item())
        state, o = {}, 0
        for i, shape in enumerate(self._shapes.values()):
            size = int(np.prod(shape))
            state[i] = {"step": torch.tensor(step), "exp_avg": self.exp_avg[o:o + size].view(shape).clone(),
                        "exp_avg_sq": self.exp_avg_sq[o:o + size].view(shape).clone()}
            o += size
        group = {"lr": self.learning_rate, "betas": self.betas, "eps": self.eps, "weight_decay": 0, "amsgrad": False,
                 "maximize": False, "foreach": None, "capturable": False, "differentiable": False, "fused": None,
                 "params": list(range(len(self._shapes)))}
        return {"state": state, "param_groups": [group]}

    def load_optimizer_state_dict(self, sd):
        """The inverse: moments and step count from a `torch.optim.Adam` state dict over the same parameters (every
        parameter's `step` must agree; an empty state is a fresh optimiser), and the learning rate of its param group.  The
        running products of the betas are rebuilt by `step` float64 multiplications, as the kernel builds them."""
        who = "DevicePPO.load_optimizer_state_dict: "
        try:
            state, groups = sd["state"], sd["param_groups"]
        except (TypeError, KeyError):
            raise ValueError(who + "not an optimiser state dict")
        n = len(self._shapes)
        if len(groups) != 1 or list(groups[0].get("params", ())) != list(range(n)):
            raise ValueError(who + "one param group over the %d parameters is expected" % n)
        if groups[0].get("weight_decay", 0) or groups[0].get("amsgrad", False) or groups[0].get("maximize", False):
            raise ValueError(who + "weight decay, amsgrad and maximize are not built")
        if len(state) not in (0, n):
            raise ValueError(who + "state for none or all of the %d parameters is expected" % n)
        steps = {int(float(state[i]["step"])) for i in state} or {0}
        if len(steps) != 1 or min(steps) < 0:
            raise ValueError(who + "every parameter must carry the same non-negative step")
        for i, shape in enumerate(self._shapes.values()):
            if state and any(tuple(state[i][k].shape) != shape or state[i][k].dtype != torch.float32
                             for k in ("exp_avg", "exp_avg_sq")):
                raise ValueError(who + "parameter %d: float32 moments of shape %s are expected" % (i, shape))
        step, o = steps.pop(), 0
        for i, shape in enumerate(self._shapes.values()):
            size = int(np.prod(shape))
            for name, mine in (("exp_avg", self.exp_avg), ("exp_avg_sq", self.exp_avg_sq)):
                if state:
                    mine[o:o + size].copy_(state[i][name].reshape(-1))
                else:
                    mine[o:o + size].zero_()
            o += size
        pw = [1.0, 1.0]
        for _ in range(step):
            pw[0] *= self.betas[0]
            pw[1] *= self.betas[1]
        self._step.fill_(step)
        self._beta_pow.copy_(torch.tensor(pw, dtype=torch.float64))
        if "lr" in groups[0]:
            self.set_learning_rate(groups[0]["lr"])
