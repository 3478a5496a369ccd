"""The device policy forward: the reference's late-fusion actor-critic on learner rows, between `env.step` and `ro.store`.

`DevicePolicy` is the reference's `NeuralNet.forward` under `torch.no_grad()` (gpudrive/networks/late_fusion.py:170-210, the
middle of the rollout loop gpudrive/integrations/puffer/ppo.py:129-199) as one C call (`gd_policy_forward`, three launches,
csrc/policy.hip): both set embedders on float32 MFMA with the LayerNorm, the tanh, the second layer and the max-pool in
registers, so none of the [N, 200, 64] and [N, A-1, 64] intermediates exists; then 192 -> 128 -> n_actions + 1 over tiles of
32 rows; then the action rule.  Float32 throughout: the logprob stored in the rollout is later compared with torch's own
float32 recomputation in the PPO ratio.

    pol = DevicePolicy.from_state_dict(net.state_dict(), max_agents=128, ego_width=6)   # 9: ConditionedLearnerEnv rows
    while not ro.full:
        u = torch.rand(N, device="cuda", generator=g)
        actions, logprob, entropy, value = pol(obs, u)        # or pol(obs, deterministic=True); out=... reuses buffers
        ro.store(obs, value, actions, logprob, rewards, terminals, masks)
        obs, rewards, terminals, truncations, masks = env.step(actions)

DROPOUT.  Without a rule the forward is the module in eval mode: dropout is the identity.  The reference's rollout does not
call `.eval()` and its yaml has dropout 0.01, so its own rollout forward drops 1 % of the embedder activations and of the
hidden vector at random.  `dropout_rule=DropoutRule(p, seed)` (dropout.py) gives that forward: the four sites are masked in
the kernels by this project's counter-based rule (csrc/dropout_rule.hpp; `nn.Dropout`'s own stream cannot be reproduced),
on every call while `pol.training` is true -- `deterministic=True` does not switch the masks off, as it does not in the
reference.  `pol.eval()` is the unmasked forward again, `pol.train()` the masked one.

The network rule and the action rule are stated in include/gpudrive_amd.h (`gd_policy`) and csrc/policy_rule.hpp.  The
draw is this project's: `torch.multinomial`'s random stream cannot be reproduced, so the action is a function of one
uniform u in [0, 1) per row -- the first k whose running sum of exp(l - max l), in ascending k, exceeds u times the whole sum.
The max-pools run over ALL A - 1 partner rows and all 200 road rows, padding rows included, as the reference's do.
Observations must be finite.

`TrainablePolicy` (below) is the training side: the same network as a differentiable torch module, its forward for given
actions (`gd_policy_evaluate`) and its backward to parameter gradients (`gd_policy_backward`, csrc/policy_grad.hip) in HIP.

Not here: a bf16 or fp8 forward, a gradient with respect to the observations, LSTM state, GELU, `vbd_in_obs`, more than 1024
actions.  The losses, gradient clipping and the optimiser on the device are `gpudrive_lab_amd.ppo.DevicePPO` (ppo.py), which
runs the whole minibatch update as one C call; `TrainablePolicy` remains for callers who write those lines in torch."""
import ctypes as C

import numpy as np
import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import _capi
from .dropout import check_rule

INPUT_DIM, HIDDEN_DIM, ROADS, ROAD_K, PARTNER_K = 64, 128, 200, 13, 6
FEATURES = 3 * INPUT_DIM
MAX_ACTIONS = 1024
MAX_ROWS = 1 << 20
EMBEDDERS = ("ego_embed", "partner_embed", "road_map_embed")


def _is_int(v):
    return isinstance(v, int) and not isinstance(v, bool)


def obs_width(max_agents, ego_width):
    return ego_width + PARTNER_K * (max_agents - 1) + ROAD_K * ROADS


def expected_shapes(ego_width, n_actions):
    """The state dict of the supported module, by the reference's own names, in the order the packer concatenates it."""
    shapes = {}
    for name, k in zip(EMBEDDERS, (ego_width, PARTNER_K, ROAD_K)):
        shapes[name + ".0.weight"], shapes[name + ".0.bias"] = (INPUT_DIM, k), (INPUT_DIM,)
        shapes[name + ".1.weight"], shapes[name + ".1.bias"] = (INPUT_DIM,), (INPUT_DIM,)
        shapes[name + ".4.weight"], shapes[name + ".4.bias"] = (INPUT_DIM, INPUT_DIM), (INPUT_DIM,)
    shapes["shared_embed.0.weight"], shapes["shared_embed.0.bias"] = (HIDDEN_DIM, FEATURES), (HIDDEN_DIM,)
    shapes["actor.weight"], shapes["actor.bias"] = (n_actions, HIDDEN_DIM), (n_actions,)
    shapes["critic.weight"], shapes["critic.bias"] = (1, HIDDEN_DIM), (1,)
    return shapes


def check_policy_args(state_dict, max_agents, ego_width, act_func="tanh", vbd_in_obs=False, who="DevicePolicy: "):
    """Everything `DevicePolicy` refuses, checked on the host before anything reaches the device (ValueError).  Returns
    n_actions."""
    if act_func != "tanh":
        raise ValueError(who + "act_func %r is not built (tanh only)" % (act_func,))
    if vbd_in_obs:
        raise ValueError(who + "vbd_in_obs is not built")
    if not _is_int(max_agents) or max_agents not in (64, 128):
        raise ValueError(who + "max_agents must be 64 or 128, got %r" % (max_agents,))
    if not _is_int(ego_width) or ego_width not in (6, 9):
        raise ValueError(who + "ego_width must be 6 or 9, got %r" % (ego_width,))
    if not hasattr(state_dict, "keys") or not hasattr(state_dict, "__getitem__"):
        raise ValueError(who + "state_dict must be a mapping of names to tensors")
    keys = set(state_dict.keys())
    if "actor.weight" not in keys:
        raise ValueError(who + "missing key 'actor.weight'")
    aw = state_dict["actor.weight"]
    if not isinstance(aw, torch.Tensor) or aw.dim() != 2:
        raise ValueError(who + "actor.weight must be a [n_actions, %d] tensor" % HIDDEN_DIM)
    n_actions = int(aw.shape[0])
    if not 1 <= n_actions <= MAX_ACTIONS:
        raise ValueError(who + "n_actions must be in [1, %d], got %d" % (MAX_ACTIONS, n_actions))
    want = expected_shapes(ego_width, n_actions)
    missing, extra = sorted(set(want) - keys), sorted(keys - set(want))
    if missing:
        raise ValueError(who + "missing key(s) %s" % ", ".join(map(repr, missing)))
    if extra:
        raise ValueError(who + "unexpected key(s) %s" % ", ".join(map(repr, extra)))
    for name, shape in want.items():
        t = state_dict[name]
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape:
            raise ValueError(who + "%s must be a tensor of shape %s (input_dim %d, hidden_dim %d), got %s"
                             % (name, shape, INPUT_DIM, HIDDEN_DIM, tuple(t.shape) if isinstance(t, torch.Tensor) else type(t)))
        if t.dtype != torch.float32:
            raise ValueError(who + "%s must be float32, got %s" % (name, t.dtype))
        if not t.is_contiguous():
            raise ValueError(who + "%s must be contiguous" % name)
    return n_actions


def _acc_row(r, h):
    return (r & 3) + 8 * (r >> 2) + 4 * h


def pack_index(ego_width, n_actions):
    """The layout of `gd_policy.blob` as an index: blob = flat[pack_index], where flat is the state dict's tensors flattened
    and concatenated in `expected_shapes` order, followed by one zero (the index of every padding element).  int64 numpy."""
    shapes = expected_shapes(ego_width, n_actions)
    base, o = {}, 0
    for name, shape in shapes.items():
        base[name] = o
        o += int(np.prod(shape))
    zero = o
    lane = np.arange(64)
    c, h = lane & 31, lane >> 5
    acc = np.array([[_acc_row(r, hh) for hh in (0, 1)] for r in range(16)])  # [r][h]
    parts = []

    def nat(name):
        parts.append(base[name] + np.arange(int(np.prod(shapes[name]))))

    e = EMBEDDERS[0]
    nat(e + ".0.weight"), nat(e + ".0.bias"), nat(e + ".1.weight"), nat(e + ".1.bias")
    parts.append((base[e + ".4.weight"] + np.arange(64)[None, :] * 64 + np.arange(64)[:, None]).reshape(-1))  # [in][out]
    nat(e + ".4.bias")
    for e, k, ks in ((EMBEDDERS[1], PARTNER_K, 3), (EMBEDDERS[2], ROAD_K, 7)):
        t, s = np.arange(2)[:, None, None], np.arange(ks)[None, :, None]
        col = ks * h[None, None, :] + s + 0 * t
        idx = base[e + ".0.weight"] + (32 * t + c[None, None, :]) * k + col
        parts.append(np.where(col < k, idx, zero).reshape(-1))
        nat(e + ".0.bias"), nat(e + ".1.weight"), nat(e + ".1.bias")
        t2, t, r = np.arange(2)[:, None, None, None], np.arange(2)[None, :, None, None], np.arange(16)[None, None, :, None]
        col = 32 * t + acc[r, h[None, None, None, :]]
        parts.append((base[e + ".4.weight"] + (32 * t2 + c[None, None, None, :]) * 64 + col).reshape(-1))
        nat(e + ".4.bias")
    t, s = np.arange(4)[:, None, None], np.arange(96)[None, :, None]
    parts.append((base["shared_embed.0.weight"] + (32 * t + c[None, None, :]) * FEATURES + 96 * h[None, None, :] + s).reshape(-1))
    nat("shared_embed.0.bias")
    tiles = (n_actions + 1 + 31) // 32
    i, t, r = np.arange(tiles)[:, None, None, None], np.arange(4)[None, :, None, None], np.arange(16)[None, None, :, None]
    a = 32 * i + c[None, None, None, :] + 0 * t + 0 * r
    col = 32 * t + acc[r, h[None, None, None, :]] + 0 * i
    idx = np.where(a < n_actions, base["actor.weight"] + a * HIDDEN_DIM + col,
                   np.where(a == n_actions, base["critic.weight"] + col, zero))
    parts.append(idx.reshape(-1))
    a = np.arange(tiles * 32)
    parts.append(np.where(a < n_actions, base["actor.bias"] + a, np.where(a == n_actions, base["critic.bias"], zero)))
    return np.concatenate([np.asarray(p, dtype=np.int64).reshape(-1) for p in parts])


def live_rows_scratch_ints(n):
    """The int32 words of `gd_live_rows`' scratch for n rows: one per block of `_capi.LIVE_ROWS_BLOCK` rows."""
    return (n + _capi.LIVE_ROWS_BLOCK - 1) // _capi.LIVE_ROWS_BLOCK


class LiveRows:
    """A device-resident list of rows: `rows` int32 [N], of which the first `count[0]` are the list, ascending; `count` int32
    [1]; `scratch`, which `live_rows` needs.  Nothing on the host knows the length.  A new one lists no row (count 0).
    new: who makes the three arrays, as new(name, shape, dtype, fill, device) (fill None: need not be initialised)."""

    def __init__(self, n, device, new=None):
        if not _is_int(n) or not 1 <= n <= MAX_ROWS:
            raise ValueError("LiveRows: N must be an int in [1, %d], got %r" % (MAX_ROWS, n))
        if new is None:
            new = lambda name, shape, dt, fill, dev: (torch.empty(shape, dtype=dt, device=dev) if fill is None  # noqa: E731
                                                      else torch.full(shape, fill, dtype=dt, device=dev))
        self.n = n
        self.rows = new("rows", (n,), torch.int32, None, device)
        self.count = new("rows_count", (1,), torch.int32, 0, device)
        self.scratch = new("rows_scratch", (live_rows_scratch_ints(n),), torch.int32, None, device)

    @staticmethod
    def nbytes(n):
        """Bytes a LiveRows of n rows holds: rows, count and scratch."""
        return 4 * (n + 1 + live_rows_scratch_ints(n))


def live_rows(mask, out=None):
    """mask: a contiguous bool or uint8 tensor [N] on the GPU, 1 <= N <= 2^20; a byte that is not zero is a live row.  Returns
    the `LiveRows` of the rows whose byte is set, in ascending order (`gd_live_rows`, csrc/live_rows.hip).  out: a LiveRows of
    the same N and device to be overwritten; then nothing is allocated.  Two launches on torch's current stream, no host
    synchronisation, no atomics: equal masks give equal bytes.  `rows[count:]` is not written."""
    who = "live_rows: "
    if not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.bool, torch.uint8) or mask.dim() != 1 \
            or not mask.is_contiguous():
        raise ValueError(who + "mask must be a contiguous bool or uint8 tensor of shape [N]")
    n = int(mask.shape[0])
    if not 1 <= n <= MAX_ROWS:
        raise ValueError(who + "N must be in [1, %d], got %d" % (MAX_ROWS, n))
    if mask.device.type != "cuda":
        raise ValueError(who + "mask must be on the GPU (there is no host path), got %s" % mask.device)
    if out is None:
        out = LiveRows(n, mask.device)
    elif not isinstance(out, LiveRows) or out.n != n or out.rows.device != mask.device:
        raise ValueError(who + "out must be a LiveRows of N = %d on %s" % (n, mask.device))
    with torch.cuda.device(mask.device):
        stream = C.c_void_p(torch.cuda.current_stream(mask.device).cuda_stream)
        _capi.check(_capi.lib().gd_live_rows(mask.data_ptr(), n, out.rows.data_ptr(), out.count.data_ptr(), out.scratch.data_ptr(),
                                             stream), "gd_live_rows")
    return out


def owned_rows_positions(n, n_policies):
    """The positions of an owned list's arrays: n rows and 32 of padding per policy."""
    return n + _capi.OWNED_ROWS_ALIGN * n_policies


class OwnedRows:
    """A device-resident row list with a segment per policy (`gd_owned_rows`): `rows` int32 [N + 32 P]; `start` int32 [P + 1],
    every entry a multiple of 32; `count` int32 [P]; segment p is rows[start[p] : start[p] + count[p]], ascending, and the
    positions from there to start[p + 1] hold -1; `scratch`, which `owned_rows` needs.  Nothing on the host knows the lengths.
    A new one lists no row.  new: who makes the four arrays, as for `LiveRows`."""

    def __init__(self, n, n_policies, device, new=None):
        if not _is_int(n) or not 1 <= n <= MAX_ROWS:
            raise ValueError("OwnedRows: N must be an int in [1, %d], got %r" % (MAX_ROWS, n))
        if not _is_int(n_policies) or not 1 <= n_policies <= _capi.POLICY_SET_MAX:
            raise ValueError("OwnedRows: the number of policies must be an int in [1, %d], got %r" % (_capi.POLICY_SET_MAX, n_policies))
        if new is None:
            new = lambda name, shape, dt, fill, dev: (torch.empty(shape, dtype=dt, device=dev) if fill is None  # noqa: E731
                                                      else torch.full(shape, fill, dtype=dt, device=dev))
        self.n, self.n_policies = n, n_policies
        self.rows = new("owned_rows", (owned_rows_positions(n, n_policies),), torch.int32, None, device)
        self.start = new("owned_start", (n_policies + 1,), torch.int32, 0, device)
        self.count = new("owned_count", (n_policies,), torch.int32, 0, device)
        self.scratch = new("owned_scratch", (n_policies * live_rows_scratch_ints(n),), torch.int32, None, device)

    @staticmethod
    def nbytes(n, n_policies):
        """Bytes an OwnedRows holds: rows, start, count and scratch."""
        return 4 * (owned_rows_positions(n, n_policies) + 2 * n_policies + 1 + n_policies * live_rows_scratch_ints(n))


def owned_rows(mask, owner, n_policies=None, out=None):
    """mask: a contiguous bool or uint8 tensor [N] on the GPU (a byte that is not zero is a live row); owner: a contiguous uint8
    tensor [N] on the same device, the policy index of every row (a row whose owner is >= n_policies is listed nowhere).
    Returns the `OwnedRows` (`gd_owned_rows`, csrc/owned_rows.hip).  out: an OwnedRows of the same N, number of policies and
    device to be overwritten (n_policies may then be omitted); then nothing is allocated.  Two launches on torch's current
    stream, no host synchronisation, no atomics: equal input gives equal bytes.  rows[start[P]:] is not written."""
    who = "owned_rows: "
    if not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.bool, torch.uint8) or mask.dim() != 1 \
            or not mask.is_contiguous():
        raise ValueError(who + "mask must be a contiguous bool or uint8 tensor of shape [N]")
    n = int(mask.shape[0])
    if not 1 <= n <= MAX_ROWS:
        raise ValueError(who + "N must be in [1, %d], got %d" % (MAX_ROWS, n))
    if mask.device.type != "cuda":
        raise ValueError(who + "mask must be on the GPU (there is no host path), got %s" % mask.device)
    if not isinstance(owner, torch.Tensor) or owner.dtype != torch.uint8 or tuple(owner.shape) != (n,) or not owner.is_contiguous() \
            or owner.device != mask.device:
        raise ValueError(who + "owner must be a contiguous uint8 tensor of shape [%d] on %s" % (n, mask.device))
    if n_policies is None and isinstance(out, OwnedRows):
        n_policies = out.n_policies
    if not _is_int(n_policies) or not 1 <= n_policies <= _capi.POLICY_SET_MAX:
        raise ValueError(who + "n_policies must be an int in [1, %d], got %r" % (_capi.POLICY_SET_MAX, n_policies))
    if out is None:
        out = OwnedRows(n, n_policies, mask.device)
    elif not isinstance(out, OwnedRows) or out.n != n or out.n_policies != n_policies or out.rows.device != mask.device:
        raise ValueError(who + "out must be an OwnedRows of N = %d and %d policies on %s" % (n, n_policies, mask.device))
    with torch.cuda.device(mask.device):
        stream = C.c_void_p(torch.cuda.current_stream(mask.device).cuda_stream)
        _capi.check(_capi.lib().gd_owned_rows(mask.data_ptr(), owner.data_ptr(), n, n_policies, out.rows.data_ptr(),
                                              out.start.data_ptr(), out.count.data_ptr(), out.scratch.data_ptr(), None, stream),
                    "gd_owned_rows")
    return out


def check_policy_set(policies, who):
    """The policies of one `PolicySet`: 1 to 8 `DevicePolicy` of one shape (ValueError otherwise)."""
    policies = tuple(policies)
    if not 1 <= len(policies) <= _capi.POLICY_SET_MAX:
        raise ValueError(who + "a set holds 1 to %d policies, got %d" % (_capi.POLICY_SET_MAX, len(policies)))
    for p in policies:
        if not isinstance(p, DevicePolicy):
            raise ValueError(who + "every policy must be a DevicePolicy, got %s" % type(p).__name__)
    first = policies[0]
    for i, p in enumerate(policies):
        for k in ("max_agents", "ego_width", "n_actions"):
            if getattr(p, k) != getattr(first, k):
                raise ValueError(who + "the policies of a set share one shape: policy %d has %s %d, policy 0 has %d"
                                 % (i, k, getattr(p, k), getattr(first, k)))
    return policies


class PolicySet:
    """1 to 8 `DevicePolicy` of one shape (max_agents, ego_width, n_actions) on one device, and the position-indexed scratch
    of the forward on an owned list (`gd_policy_forward_owned`), in which every row is computed with the weights of its owner:
    three launches whatever the number of policies.  The policies' blobs are read in place, so the set follows an optimiser
    that moves them.  The scratch belongs to the set (it grows with the largest N seen): a set serves ONE stream at a time."""

    def __init__(self, policies):
        self.policies = check_policy_set(policies, "PolicySet: ")
        first = self.policies[0]
        for p in self.policies:
            if p.device != first.device:
                raise ValueError("PolicySet: the policies are on %s and %s" % (first.device, p.device))
        self.device, self.max_agents, self.ego_width, self.n_actions = first.device, first.max_agents, first.ego_width, first.n_actions
        self.obs_width = first.obs_width
        self._features = self._logits = None
        self._rows = 0

    def __len__(self):
        return len(self.policies)

    @staticmethod
    def scratch_nbytes(n, n_policies, n_actions):
        """Bytes of the features and logits scratch of a forward on N rows."""
        return owned_rows_positions(n, n_policies) * (FEATURES + n_actions) * 4

    def _struct(self, n, new=None):
        """The gd_policy_set of a forward on n rows; the scratch grows here, and nowhere else.  new: who makes the scratch of
        THIS call instead (as for `LiveRows`; kept by the caller)."""
        q = owned_rows_positions(n, len(self.policies))
        if new is not None:
            features = new("set_features", (q, FEATURES), torch.float32, None, self.device)
            logits = new("set_logits", (q, self.n_actions), torch.float32, None, self.device)
        else:
            if n > self._rows:
                self._features = torch.empty((q, FEATURES), dtype=torch.float32, device=self.device)
                self._logits = torch.empty((q, self.n_actions), dtype=torch.float32, device=self.device)
                self._rows = n
            features, logits = self._features, self._logits
        s = _capi.GdPolicySet()
        s.n_policies = len(self.policies)
        for i, p in enumerate(self.policies):
            g = s.policy[i]
            g.num_rows, g.max_agents, g.ego_width, g.n_actions = n, p.max_agents, p.ego_width, p.n_actions
            g.blob, g.blob_floats = p.blob.data_ptr(), p.blob.numel()
        s.features, s.logits = features.data_ptr(), logits.data_ptr()
        s._keep = (features, logits)
        return s

    def __call__(self, obs, rows, u=None, deterministic=False, out=None, logits_out=None):
        """obs [N, obs_width] float32, contiguous, on the device; rows: an `OwnedRows` of this N and this number of policies
        (`owned_rows(mask, owner)`).  u [N] float32 in [0, 1) (required unless deterministic).  Returns (actions int64 [N],
        logprob, entropy, value float32 [N]): index r of a row listed under policy p holds the bits `policies[p](obs)` gives
        that row; out= and logits_out keep their bytes at rows that are not listed, and with out=None the fresh outputs are
        zero there.  Always the unmasked forward: a dropout rule on a policy is neither consulted nor advanced.  Three launches
        on torch's current stream, no host synchronisation; with out= and an N seen before, no allocation either."""
        first, who = self.policies[0], "PolicySet: "
        if not isinstance(obs, torch.Tensor) or obs.dim() != 2 or obs.shape[1] != self.obs_width:
            raise ValueError(who + "obs must be a [N, %d] tensor (max_agents %d, ego_width %d)"
                             % (self.obs_width, self.max_agents, self.ego_width))
        n = int(obs.shape[0])
        if not 1 <= n <= MAX_ROWS:
            raise ValueError(who + "N must be in [1, %d], got %d" % (MAX_ROWS, n))
        if not isinstance(rows, OwnedRows) or rows.n != n or rows.n_policies != len(self.policies) or rows.rows.device != self.device:
            raise ValueError(who + "rows must be an OwnedRows of N = %d and %d policies on %s" % (n, len(self.policies), self.device))
        first._tensor("obs", obs, torch.float32, (n, self.obs_width))
        deterministic = bool(deterministic)
        if u is None:
            if not deterministic:
                raise ValueError(who + "u is required unless deterministic=True")
        else:
            first._tensor("u", u, torch.float32, (n,))
        f = torch.float32
        want = (((n,), torch.int64), ((n,), f), ((n,), f), ((n,), f))
        if out is None:
            out = tuple(torch.zeros(shape, dtype=dt, device=self.device) for shape, dt in want)
        else:
            if not isinstance(out, (tuple, list)) or len(out) != 4:
                raise ValueError(who + "out must be the four tensors (actions, logprob, entropy, value)")
            out = tuple(first._tensor("out " + name, o, dt, shape) for name, o, (shape, dt) in zip(DevicePolicy.OUT_NAMES, out, want))
        if logits_out is not None:
            first._tensor("logits_out", logits_out, f, (n, self.n_actions))
        s = self._struct(n)
        with torch.cuda.device(self.device):
            stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            _capi.check(_capi.lib().gd_policy_forward_owned(
                C.byref(s), obs.data_ptr(), None if u is None else u.data_ptr(), int(deterministic), out[0].data_ptr(),
                out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), None if logits_out is None else logits_out.data_ptr(),
                rows.rows.data_ptr(), rows.start.data_ptr(), rows.count.data_ptr(), stream), "gd_policy_forward_owned")
        return out


class DevicePolicy:
    def __init__(self, state_dict, max_agents=128, ego_width=6, *, device="cuda", act_func="tanh", vbd_in_obs=False,
                 dropout_rule=None):
        """state_dict: the reference module's (`ego_embed.0/1/4`, `partner_embed.0/1/4`, `road_map_embed.0/1/4`: Linear,
        LayerNorm with affine, Linear; `shared_embed.0`, `actor`, `critic`), float32, with input_dim 64, hidden_dim 128 and
        1 <= n_actions <= 1024.  max_agents: 64 or 128.  ego_width: 6, or 9 for reward-conditioned rows.  Anything else --
        other widths, an activation other than tanh, vbd_in_obs, more than 1024 actions (the 8000-entry delta table), a
        missing or extra key, a wrong shape or dtype -- is a ValueError raised before anything reaches the device.
        dropout_rule: None (the module in eval mode) or a `DropoutRule` on the same device (see the module docstring)."""
        self.n_actions = check_policy_args(state_dict, max_agents, ego_width, act_func, vbd_in_obs)
        check_rule(dropout_rule, "DevicePolicy: ")
        self.max_agents, self.ego_width = max_agents, ego_width
        self.obs_width = obs_width(max_agents, ego_width)
        try:
            dev = torch.device(device)
        except (RuntimeError, TypeError) as e:
            raise ValueError("DevicePolicy: device: %s" % e)
        if dev.type != "cuda":
            raise ValueError("DevicePolicy: the policy runs on the GPU (there is no host path), got device %r" % (device,))
        self._L = _capi.lib()
        self.device = dev if dev.index is not None else torch.device("cuda", torch.cuda.current_device())
        self.dropout_rule = check_rule(dropout_rule, "DevicePolicy: ", self.device)
        self.training = True
        self._names = tuple(expected_shapes(ego_width, self.n_actions))
        self._index = torch.from_numpy(pack_index(ego_width, self.n_actions)).to(self.device)
        self._zero = torch.zeros(1, dtype=torch.float32, device=self.device)
        self.blob = torch.empty(self._index.numel(), dtype=torch.float32, device=self.device)
        self._features = self._logits = None
        self._rows = 0
        self._pack(state_dict)

    @classmethod
    def from_state_dict(cls, state_dict, max_agents=128, ego_width=6, **kw):
        return cls(state_dict, max_agents, ego_width, **kw)

    def train(self, mode=True):
        """With a dropout rule: mask every call (the default, as the reference's rollout does).  Returns self."""
        self.training = bool(mode)
        return self

    def eval(self):
        """The unmasked forward, whether or not there is a dropout rule.  Returns self."""
        return self.train(False)

    def _pack(self, sd):
        with torch.no_grad():
            flat = torch.cat([sd[k].detach().to(self.device).reshape(-1) for k in self._names] + [self._zero])
            torch.index_select(flat, 0, self._index, out=self.blob)

    def load_state_dict(self, state_dict):
        """Re-pack after an optimiser step: the same keys, shapes and dtypes (ValueError otherwise).  For tensors already on
        the device this is a concatenation and one gather on the device, on torch's current stream."""
        if check_policy_args(state_dict, self.max_agents, self.ego_width) != self.n_actions:
            raise ValueError("DevicePolicy.load_state_dict: n_actions must stay %d" % self.n_actions)
        self._pack(state_dict)

    def _tensor(self, name, t, dtype, shape):
        if not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != tuple(shape) or t.device != self.device \
                or not t.is_contiguous():
            raise ValueError("DevicePolicy: %s must be a contiguous %s tensor of shape %s on %s" % (name, dtype, tuple(shape), self.device))
        return t

    def _struct(self, n):
        """The gd_policy of a forward on n rows; the features and logits scratch grows here, and nowhere else."""
        if n > self._rows:
            self._features = torch.empty((n, FEATURES), dtype=torch.float32, device=self.device)
            self._logits = torch.empty((n, self.n_actions), dtype=torch.float32, device=self.device)
            self._rows = n
        p = _capi.GdPolicy()
        p.num_rows, p.max_agents, p.ego_width, p.n_actions = n, self.max_agents, self.ego_width, self.n_actions
        p.blob, p.blob_floats = self.blob.data_ptr(), self.blob.numel()
        p.features, p.logits = self._features.data_ptr(), self._logits.data_ptr()
        return p

    OUT_NAMES = ("actions", "logprob", "entropy", "value")

    def __call__(self, obs, u=None, deterministic=False, out=None, logits_out=None, rows=None):
        """obs [N, obs_width] float32, contiguous, on the device.  u [N] float32 in [0, 1) (required unless deterministic).
        Returns (actions int64 [N], logprob, entropy, value float32 [N]).  out: those four tensors of an earlier call, to be
        overwritten (every listed row is written: without rows= that is every byte); logits_out: [N, n_actions] float32 to
        receive the logits.  rows: None for all N rows, or a `LiveRows` of this N (`live_rows(mask)`): the forward then runs on
        the listed rows only (`gd_policy_forward_rows`), reads obs[r] and u[r] and writes index r of every output with the bits
        the full forward gives that row; out= and logits_out keep their bytes at rows that are not listed, and with out=None
        the fresh outputs are zero there.  The list's length stays on the device.  Three launches on
        torch's current stream, no host synchronisation; with out= and an N seen before, no allocation either, so the call can
        be captured in a graph.  With a dropout rule and `training`, the call consumes the rule's call index and advances
        it on the device.  The features and logits scratch belongs to the object (it grows with the largest N seen), so
        a DevicePolicy serves ONE stream at a time: calls on two streams need two objects or an event between them."""
        if not isinstance(obs, torch.Tensor) or obs.dim() != 2 or obs.shape[1] != self.obs_width:
            raise ValueError("DevicePolicy: obs must be a [N, %d] tensor (max_agents %d, ego_width %d)"
                             % (self.obs_width, self.max_agents, self.ego_width))
        n = int(obs.shape[0])
        if not 1 <= n <= MAX_ROWS:
            raise ValueError("DevicePolicy: N must be in [1, %d], got %d" % (MAX_ROWS, n))
        if rows is not None and (not isinstance(rows, LiveRows) or rows.n != n):
            raise ValueError("DevicePolicy: rows must be a LiveRows of N = %d (live_rows(mask)), got %s"
                             % (n, "one of N = %d" % rows.n if isinstance(rows, LiveRows) else type(rows).__name__))
        self._tensor("obs", obs, torch.float32, (n, self.obs_width))
        if rows is not None and rows.rows.device != self.device:
            raise ValueError("DevicePolicy: rows is on %s, the policy on %s" % (rows.rows.device, self.device))
        deterministic = bool(deterministic)
        if u is None:
            if not deterministic:
                raise ValueError("DevicePolicy: u is required unless deterministic=True")
        else:
            self._tensor("u", u, torch.float32, (n,))
        f = torch.float32
        want = (((n,), torch.int64), ((n,), f), ((n,), f), ((n,), f))
        if out is None:
            make = torch.empty if rows is None else torch.zeros  # (rows that are not listed are not written)
            out = tuple(make(shape, dtype=dt, device=self.device) for shape, dt in want)
        else:
            if not isinstance(out, (tuple, list)) or len(out) != 4:
                raise ValueError("DevicePolicy: out must be the four tensors (actions, logprob, entropy, value)")
            out = tuple(self._tensor("out " + name, o, dt, shape) for name, o, (shape, dt) in zip(self.OUT_NAMES, out, want))
        if logits_out is not None:
            self._tensor("logits_out", logits_out, f, (n, self.n_actions))
        p = self._struct(n)
        with torch.cuda.device(self.device):
            stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            args = (obs.data_ptr(), None if u is None else u.data_ptr(), int(deterministic), out[0].data_ptr(), out[1].data_ptr(),
                    out[2].data_ptr(), out[3].data_ptr(), None if logits_out is None else logits_out.data_ptr(), stream)
            masked = self.dropout_rule is not None and self.training
            if rows is not None:
                d = C.byref(self.dropout_rule.struct()) if masked else None
                _capi.check(self._L.gd_policy_forward_rows(C.byref(p), d, *args[:-1], rows.rows.data_ptr(), rows.count.data_ptr(),
                                                           stream), "gd_policy_forward_rows")
            elif masked:
                d = self.dropout_rule.struct()
                _capi.check(self._L.gd_policy_forward_dropout(C.byref(p), C.byref(d), *args), "gd_policy_forward_dropout")
            else:
                _capi.check(self._L.gd_policy_forward(C.byref(p), *args), "gd_policy_forward")
        return out


DEFAULT_PARTIALS = 256
MAX_PARTIALS = 1024
ROWSTAT = 8         # floats per row of the backward's scratch (csrc/policy_grad.hip)
_ALLOCATIONS = 64   # an upper bound on the tensors one forward plus backward allocates; torch rounds each up to 512 bytes


def grad_floats(ego_width, n_actions):
    """The number of parameters: the length of the flat gradient, in `expected_shapes` order."""
    return sum(int(np.prod(s)) for s in expected_shapes(ego_width, n_actions).values())


class _Evaluate(torch.autograd.Function):
    """gd_policy_evaluate forward, gd_policy_backward backward.  What the backward needs beyond the inputs -- the flat
    weights, the features, the logits and the pool winners -- belongs to this call's context, not to the module."""

    @staticmethod
    def forward(ctx, mod, obs, action, *params):
        n, na, dev, f = int(obs.shape[0]), mod.n_actions, obs.device, torch.float32
        L = _capi.lib()
        with torch.no_grad():
            flat = torch.cat([p.reshape(-1) for p in params] + [mod._zero])
            blob = torch.index_select(flat, 0, mod._index)
        features = torch.empty((n, FEATURES), dtype=f, device=dev)
        logits = torch.empty((n, na), dtype=f, device=dev)
        winners = torch.empty((n, 2 * INPUT_DIM), dtype=torch.uint8, device=dev)
        logprob, entropy, value = (torch.empty(n, dtype=f, device=dev) for _ in range(3))
        p, g = mod._structs(n, features, logits, winners)
        p.blob, p.blob_floats = blob.data_ptr(), blob.numel()
        rule = mod.dropout_rule if mod.training else None
        # the call index this forward consumes belongs to this call's context: a later forward does not disturb its backward
        used = None if rule is None else torch.empty(1, dtype=torch.int64, device=dev)
        with torch.cuda.device(dev):
            stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            args = (obs.data_ptr(), action.data_ptr(), logprob.data_ptr(), entropy.data_ptr(), value.data_ptr(), stream)
            if rule is None:
                _capi.check(L.gd_policy_evaluate(C.byref(p), C.byref(g), *args), "gd_policy_evaluate")
            else:
                d = rule.struct(used)
                _capi.check(L.gd_policy_evaluate_dropout(C.byref(p), C.byref(g), C.byref(d), *args), "gd_policy_evaluate_dropout")
        ctx.save_for_backward(obs, action, *params)  # (torch's version check then catches an optimiser step before backward)
        ctx.mod, ctx.kept, ctx.drop = mod, (flat, features, logits, winners), (rule, used)
        return logprob, entropy, value

    @staticmethod
    @once_differentiable
    def backward(ctx, d_logprob, d_entropy, d_value):
        obs, action = ctx.saved_tensors[:2]
        mod = ctx.mod
        flat, features, logits, winners = ctx.kept
        n, dev, f = int(obs.shape[0]), obs.device, torch.float32
        ups = [d.to(f).contiguous() for d in (d_logprob, d_entropy, d_value)]
        total = flat.numel() - 1
        P = mod.partials
        rowstat = torch.empty((n, ROWSTAT), dtype=f, device=dev)
        partials = torch.empty((P, total), dtype=f, device=dev)
        grad = torch.empty(total, dtype=f, device=dev)
        p, g = mod._structs(n, features, logits, winners)
        g.params, g.rowstat, g.partials = flat.data_ptr(), rowstat.data_ptr(), partials.data_ptr()
        g.grad_floats, g.num_partials = total, P
        with torch.cuda.device(dev):
            stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            args = (obs.data_ptr(), action.data_ptr(), ups[0].data_ptr(), ups[1].data_ptr(), ups[2].data_ptr(), grad.data_ptr(),
                    stream)
            rule, used = ctx.drop
            if rule is None:
                _capi.check(_capi.lib().gd_policy_backward(C.byref(p), C.byref(g), *args), "gd_policy_backward")
            else:
                d = rule.struct(used)
                _capi.check(_capi.lib().gd_policy_backward_dropout(C.byref(p), C.byref(g), C.byref(d), *args),
                            "gd_policy_backward_dropout")
        views, o = [], 0
        for shape in mod._shapes:
            k = int(np.prod(shape))
            views.append(grad[o:o + k].view(shape))
            o += k
        return (None, None, None) + tuple(views)


class TrainablePolicy(nn.Module):
    """The late-fusion actor-critic as a differentiable torch module whose forward for given actions and whose backward to
    parameter gradients run in HIP: the step of the reference's update that `DeviceRollout.minibatch` feeds
    (`data.policy(obs, action=atn)` under autograd and `loss.backward()`, gpudrive/integrations/puffer/ppo.py:261-332).

        tp = TrainablePolicy.from_state_dict(net.state_dict(), max_agents=128, ego_width=6, device="cuda")
        opt = torch.optim.Adam(tp.parameters(), lr=3e-4)
        _, newlogprob, entropy, newvalue = tp(b_obs, b_actions)
        loss = ...                                  # the reference's own lines, in torch
        opt.zero_grad(); loss.backward(); torch.nn.utils.clip_grad_norm_(tp.parameters(), 0.5); opt.step()
        pol.load_state_dict(tp.state_dict())        # the rollout's DevicePolicy follows

    The parameters carry the reference module's key names and shapes, so `state_dict()` loads into and from the reference
    `NeuralNet`, and any torch optimiser works.  The logits are bit-identical to `DevicePolicy`'s for the same weights and
    observations, so evaluating the actions it sampled returns its logprob exactly: the first epoch's PPO ratio is 1.

    DROPOUT.  The reference trains in train mode with the puffer yaml's dropout 0.01 (1 % of the embedder activations and of
    the hidden vector zeroed at random, the rest scaled by 1 / 0.99).  `dropout_rule=DropoutRule(p, seed)` gives that: in
    `.train()` the forward and its backward mask the four sites by the rule (csrc/dropout_rule.hpp); in `.eval()`, and
    without a rule, they are the unmasked path.  Each forward consumes one call index of the rule and keeps it in its own
    autograd context, so two forwards before one backward still work.  The numeric `dropout` must stay 0.0: it would promise
    `nn.Dropout`'s own random stream, which cannot be reproduced.

    The max-pools pass a pooled feature's gradient to one entity, the lowest index among those that attain the float32
    maximum (torch's `max(dim=1)` makes the same choice).  `obs` gets no gradient.

    partials: P, the number of workgroups that sum over the rows (workgroup p takes rows p, p + P, ..) and of partial
    gradients the last kernel adds in order.  The sums are deterministic for a given P.  The default, 256, is one workgroup
    on each compute unit of an MI355X -- the kernel keeps its sums in registers and fits one workgroup to a unit, so more
    adds reduction work and scratch (P times the parameters, 52 MB at 91 actions) but no parallelism; fewer rows than P
    leaves the extra workgroups storing zeros."""

    def __init__(self, state_dict, max_agents=128, ego_width=6, *, dropout=0.0, partials=None, device=None, act_func="tanh",
                 vbd_in_obs=False, dropout_rule=None):
        super().__init__()
        who = "TrainablePolicy: "
        if isinstance(dropout, bool) or not isinstance(dropout, (int, float)) or dropout != 0.0:
            raise ValueError(who + "dropout must be 0.0 (nn.Dropout's random stream cannot be reproduced; pass "
                             "dropout_rule=DropoutRule(p, seed) for training-mode masks), got %r" % (dropout,))
        self.dropout_rule = check_rule(dropout_rule, who)
        if partials is None:
            partials = DEFAULT_PARTIALS
        if not _is_int(partials) or not 1 <= partials <= MAX_PARTIALS:
            raise ValueError(who + "partials must be an int in [1, %d], got %r" % (MAX_PARTIALS, partials))
        self.n_actions = check_policy_args(state_dict, max_agents, ego_width, act_func, vbd_in_obs, who=who)
        self.max_agents, self.ego_width, self.partials = max_agents, ego_width, partials
        self.obs_width = obs_width(max_agents, ego_width)
        if device is not None:
            try:
                device = torch.device(device)
            except (RuntimeError, TypeError) as e:
                raise ValueError(who + "device: %s" % e)
        shapes = expected_shapes(ego_width, self.n_actions)
        self._names, self._shapes = tuple(shapes), tuple(shapes.values())
        for name in self._names:  # e.g. ego_embed.0.weight: plain containers under the reference's names
            *path, leaf = name.split(".")
            at = self
            for part in path:
                if part not in at._modules:
                    at.add_module(part, nn.Module())
                at = at._modules[part]
            at.register_parameter(leaf, nn.Parameter(state_dict[name].detach().to(device=device, copy=True)))
        self.register_buffer("_index", torch.from_numpy(pack_index(ego_width, self.n_actions)).to(device), persistent=False)
        self.register_buffer("_zero", torch.zeros(1, dtype=torch.float32, device=device), persistent=False)

    @classmethod
    def from_state_dict(cls, state_dict, max_agents=128, ego_width=6, **kw):
        return cls(state_dict, max_agents, ego_width, **kw)

    def _structs(self, n, features, logits, winners):
        p, g = _capi.GdPolicy(), _capi.GdPolicyGrad()
        p.num_rows, p.max_agents, p.ego_width, p.n_actions = n, self.max_agents, self.ego_width, self.n_actions
        g.features, g.logits, g.winners = features.data_ptr(), logits.data_ptr(), winners.data_ptr()
        return p, g

    def nbytes(self, n):
        """An upper bound on what one forward plus backward of n rows allocates, in bytes: n times the per-row share --
        features, logits, the three outputs, the contiguous copies of their three upstream gradients, the backward's row
        scratch, in float32, and 128 winner bytes -- plus a part that does not depend on n: the flat weights, the blob, the
        flat gradient, `partials` times the gradient, the `.grad` tensors of a first backward, and the allocator's rounding."""
        G = grad_floats(self.ego_width, self.n_actions)
        per_row = 4 * (FEATURES + self.n_actions + 3 + 3 + ROWSTAT) + 2 * INPUT_DIM
        fixed = 4 * ((G + 1) + int(self._index.numel()) + G + self.partials * G + G) + 512 * _ALLOCATIONS
        return n * per_row + fixed

    def forward(self, obs, action):
        """obs [N, obs_width] float32 and action [N] int64, contiguous, on the parameters' GPU.  Returns (action, logprob,
        entropy, value) like the reference's `forward(obs, action=atn)`; logprob, entropy and value [N] float32 are
        differentiable with respect to the parameters (once).  An action outside [0, n_actions) is clamped into it, for
        memory safety only.  Three launches on torch's current stream, and three more in the backward; no host
        synchronisation.  Sampling is `DevicePolicy`'s: action is required."""
        who = "TrainablePolicy: "
        if not isinstance(obs, torch.Tensor) or obs.dim() != 2 or obs.shape[1] != self.obs_width:
            raise ValueError(who + "obs must be a [N, %d] tensor (max_agents %d, ego_width %d)"
                             % (self.obs_width, self.max_agents, self.ego_width))
        if obs.requires_grad:
            raise ValueError(who + "obs must not require grad (there is no gradient with respect to the observations)")
        n = int(obs.shape[0])
        if not 1 <= n <= MAX_ROWS:
            raise ValueError(who + "N must be in [1, %d], got %d" % (MAX_ROWS, n))
        if obs.dtype != torch.float32 or not obs.is_contiguous() or obs.device.type != "cuda":
            raise ValueError(who + "obs must be a contiguous float32 tensor on the GPU (there is no host path)")
        if not isinstance(action, torch.Tensor) or action.dtype != torch.int64 or tuple(action.shape) != (n,) \
                or action.device != obs.device or not action.is_contiguous() or action.requires_grad:
            raise ValueError(who + "action must be a contiguous int64 tensor of shape (%d,) on %s" % (n, obs.device))
        params = []
        for name, shape in zip(self._names, self._shapes):
            p = self.get_parameter(name)
            if p.device != obs.device or p.dtype != torch.float32 or tuple(p.shape) != shape or not p.is_contiguous():
                raise ValueError(who + "parameter %s must be a contiguous float32 tensor of shape %s on %s"
                                 % (name, shape, obs.device))
            params.append(p)
        if self.dropout_rule is not None and self.training:
            check_rule(self.dropout_rule, who, obs.device)
        logprob, entropy, value = _Evaluate.apply(self, obs, action, *params)
        return action, logprob, entropy, value
