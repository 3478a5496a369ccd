"""The device BC policy forward: the reference's imitation-learning model on the batches `DeviceExpertDataset` gathers.

`DeviceBCPolicy` is `EarlyFusionAttnBCNet` in eval mode (gpudrive/integrations/il/model/model.py, networks.py; the model
baselines/il/il.py trains and the closed-loop scripts run) as one C call (`gd_bc_forward`, csrc/bc_policy.hip): the token
embedders, the fusion / object / road self-attention layers with their streamed softmax, both cross attentions of the ego
token, the GMM head and the mixture rule (csrc/bc_rule.hpp).  Float32 throughout, exact-f32 MFMA over token tiles; no tensor
with an L x L extent exists anywhere -- the scores of a (sample, head, 32-query tile) live in one accumulator.

    bc = DeviceBCPolicy.from_state_dict(sd, max_agents=128, num_stack=5, num_layer=(3, 2), num_head=4,
                                        head_num_layers=2, n_components=6, clip_value=-20.0)
    obs, expert, pm, rm, data_idx = ds.batch(sel)                 # DeviceExpertDataset, unchanged
    actions = bc(obs, pm, rm, deterministic=True)                 # [B, 1, 3]
    actions = bc(obs, pm, rm, u=u, z=z)                           # the rule's draw
    ctx     = bc.context(obs, pm, rm)                             # [B, 192]
    means, cov, weights = bc.gmm_params(obs, pm, rm)              # [B,1,C,3], [B,1,C,3], [B,1,C]
    nll     = bc.nll(obs, pm, rm, expert)                         # [B] (gmm_loss's detached second value)
    stats   = bc.evaluate(ds, batch_size=512)                     # il.py:99-180's eight numbers, ONE host read
    bc.load_state_dict(sd)                                        # re-pack after a torch optimiser's step
    lr = live_rows(alive, out=lr)                                 # policy.live_rows: the rows of a [B] byte mask, on the device
    bc(obs, pm, rm, deterministic=True, out=actions, rows=lr)     # the listed rows only (gd_bc_forward_rows); the others keep
                                                                  # their bytes, every listed row gets the full forward's bits
    h = bc.hidden(obs, pm, rm, tap="ro_attn", layer=0)            # [B, A, 64]: the tapped tokens after any self-attention layer
    r = bc.read(obs, pm, rm, ProbeReadout(bc, "ro_attn", 0, other=[po], ego=[pe], labels=10))   # the forward plus the probes'
                                                                  # classes read at that layer on the way (bc_readout)

The state dict carries the reference module's own parameter names (`expected_shapes`), so a `torch.save`d reference model
loads without renaming.  The draw is this project's: the reference samples the component with `dist.Categorical` and the
action with `MultivariateNormal.sample` from torch's generator, which cannot be reproduced, so the sampled action is a
function of one uniform u in [0, 1) and three standard normals z per row (csrc/bc_rule.hpp).

A masked key's score is -FLT_MAX, not -inf, as in the reference: a sample with no valid partner attends uniformly over all
A - 1 partner tokens in `ego_ro_attn`, one with no valid road uniformly in `rg_attn` and `ego_rg_attn`.  Only the last time
index of each mask is read.  Masked entities are embedded like any other.

Scratch (the token, key and value buffers) is sized to `chunk_rows` samples and allocated once; a larger B runs chunk after
chunk on the stream inside the one C call.  `nbytes(B)` states what a call of B rows touches beyond its inputs.

Not here: the backward (`bc_train.TrainableBCPolicy`, gd_bc_backward; at either width `bc_train.TrainableBCPolicyDim`,
gd_bc_backward_dim); the gradient step with clipping and AdamW
(`bc_opt.DeviceBC`, gd_bc_update, whose `policy` is one of these and follows the optimiser in place); the closed-loop driver
(`bc_rollout.ClosedLoopBC`, gd_bc_rollout, which calls this forward once per step, or with compact=True the forward on the list
of the rows still alive);
`aux_head` / `use_tom`; non-zero dropout; `separate_attn_weights`, rotary embeddings, KV caches, causal attention;
`ContHead`, `l1_loss`, `focal_loss`; SELU; a `network_dim` other than 64 or 128; probes and read-outs at 128; bf16.

`network_dim=128` (with head_dim 64: the model of the reference's sweep, baselines/il/sweep.yaml) is the inference side at that
width: `__call__`, `context` ([B, 384]), `gmm_params`, `nll`, `evaluate`, `rows=`, `load_state_dict` and the closed-loop driver
with its attention scores, on the kernels' T = 4 instantiations (csrc/bc_policy.hip, `gd_bc_forward_dim`): 4 heads of 32 channels, every
encoder Linear 128 x 128, the GMM head behind `head.input_layer` still 64 wide.  `hidden`, `read`, `DeviceLinearProbe`,
`ProbeReadout` and the names `DeviceBC` and `TrainableBCPolicy` refuse that width (ValueError, before the device is touched);
`bc_train.TrainableBCPolicyDim` is the module that trains at it, and a policy of this class follows it with `load_state_dict`;
`bc_opt.DeviceBCDim` is the whole gradient step at it, and its `policy` is one of these that follows in place."""
import ctypes as C
import math

import numpy as np
import torch

from . import _capi

DIM, HEADS, ROADS, ROAD_K, PARTNER_K, EGO_K, ACTION_DIM = 64, 4, 200, 13, 6, 6, 3
CONTEXT = 3 * DIM
NETS = ("ego_state_net", "road_object_net", "road_graph_net")
NET_K = (EGO_K, PARTNER_K, ROAD_K)
SELF_BLOCKS = ("fusion_attn", "ro_attn", "rg_attn")
CROSS_LAYERS = ("ego_ro_attn", "ego_rg_attn")
MAX_ROWS = 1 << 20
DEFAULT_CHUNK = 128
MAX_CHUNK = 4096
EVAL_NAMES = ("test_loss", "dx_loss", "dy_loss", "dyaw_loss", "dx_std2_loss", "dy_std2_loss", "dyaw_std2_loss", "tom_loss")
WHO = "DeviceBCPolicy: "
# the reference module's keyword arguments that are accepted only at the values that are built (`check_bc_args`)
FIXED = frozenset(("network_dim", "head_dim", "network_num_layers", "act_func", "dropout", "action_dim", "time_dim", "use_tom"))


def _is_int(v):
    return isinstance(v, int) and not isinstance(v, bool)


def obs_width(max_agents):
    return EGO_K + PARTNER_K * (max_agents - 1) + ROAD_K * ROADS


def _linear(shapes, name, out, inp):
    shapes[name + ".weight"], shapes[name + ".bias"] = (out, inp), (out,)


def _norm(shapes, name, dim=DIM):
    shapes[name + ".weight"], shapes[name + ".bias"] = (dim,), (dim,)


def expected_shapes(num_stack, num_layer, head_num_layers, n_components, *, network_dim=DIM):
    """The state dict of the supported module, by the reference's own names, in the reference module's own order.
    network_dim (64 or 128) is the width of the embedders and of every attention layer; the GMM head behind
    head.input_layer (3 network_dim -> 64) is head_dim = 64 wide at either."""
    s, D = {}, network_dim
    for net, k in zip(NETS, NET_K):
        for i in range(4):  # Linear, Dropout, LayerNorm, Tanh
            _linear(s, "%s.%d" % (net, 4 * i), D, k * num_stack if i == 0 else D)
            _norm(s, "%s.%d" % (net, 4 * i + 2), D)
    for blk, n in zip(SELF_BLOCKS, (num_layer[0], num_layer[1], num_layer[1])):
        for i in range(n):
            p = "%s.%d" % (blk, i)
            _norm(s, p + ".0.module.norm", D)
            for proj in "qkvo":
                _linear(s, p + ".0.module.attention.%s_proj" % proj, D, D)
            _norm(s, p + ".1.module.0", D)
            _linear(s, p + ".1.module.1", D, D)
            _linear(s, p + ".1.module.3", D, D)
    for p in CROSS_LAYERS:
        _norm(s, p + ".0.module.q_norm", D)
        _norm(s, p + ".0.module.kv_norm", D)
        for proj in "qkvo":
            _linear(s, p + ".0.module.attention.%s_proj" % proj, D, D)
        _norm(s, p + ".1.module.0", D)
        _linear(s, p + ".1.module.1", D, D)
        _linear(s, p + ".1.module.3", D, D)
    _linear(s, "head.input_layer.0", DIM, 3 * D)
    for i in range(head_num_layers):
        _linear(s, "head.residual_block.%d.0" % i, DIM, DIM)
    _linear(s, "head.head", n_components * (2 * ACTION_DIM + 1), DIM)
    return s


def check_bc_args(state_dict, max_agents=128, num_stack=5, num_layer=(3, 2), num_head=4, head_num_layers=2, n_components=6,
                  clip_value=-20.0, *, network_dim=64, head_dim=64, network_num_layers=4, act_func="tanh", dropout=0.0,
                  action_dim=3, time_dim=1, use_tom=None, chunk_rows=DEFAULT_CHUNK, who=WHO, network_dims=(DIM,)):
    """Everything `DeviceBCPolicy` refuses, checked on the host before anything reaches the device (ValueError).  Returns
    the expected shapes.  network_dims: the widths the caller has built -- (64,) unless it says otherwise, which is what the
    backward and the optimiser say; `DeviceBCPolicy` alone passes (64, 128)."""
    if not _is_int(network_dim) or network_dim not in network_dims:
        if tuple(network_dims) == (DIM,):
            raise ValueError(who + "network_dim must be 64 (nothing else is built), got %r" % (network_dim,))
        raise ValueError(who + "network_dim must be %s (nothing else is built), got %r"
                         % (" or ".join(str(v) for v in network_dims), network_dim))
    for name, v, want in (("head_dim", head_dim, 64), ("num_head", num_head, HEADS),
                          ("network_num_layers", network_num_layers, 4), ("action_dim", action_dim, ACTION_DIM),
                          ("time_dim", time_dim, 1)):
        if not _is_int(v) or v != want:
            raise ValueError(who + "%s must be %d (nothing else is built), got %r" % (name, want, v))
    if act_func != "tanh":
        raise ValueError(who + "act_func %r is not built (tanh only)" % (act_func,))
    if isinstance(dropout, bool) or not isinstance(dropout, (int, float)) or dropout != 0.0:
        raise ValueError(who + "dropout must be 0.0 in every site (the eval-mode forward), got %r" % (dropout,))
    if use_tom is not None:
        raise ValueError(who + "use_tom / aux_head is not built, got %r" % (use_tom,))
    if not _is_int(max_agents) or max_agents not in (64, 128):
        raise ValueError(who + "max_agents must be 64 or 128, got %r" % (max_agents,))
    if not _is_int(num_stack) or not 1 <= num_stack <= 8:
        raise ValueError(who + "num_stack must be an int in [1, 8], got %r" % (num_stack,))
    if not isinstance(num_layer, (tuple, list)) or len(num_layer) != 2 or not all(_is_int(v) and 1 <= v <= 4 for v in num_layer):
        raise ValueError(who + "num_layer must be two ints in [1, 4], got %r" % (num_layer,))
    if not _is_int(head_num_layers) or not 0 <= head_num_layers <= 4:
        raise ValueError(who + "head_num_layers must be an int in [0, 4], got %r" % (head_num_layers,))
    if not _is_int(n_components) or not 1 <= n_components <= 16:
        raise ValueError(who + "n_components must be an int in [1, 16], got %r" % (n_components,))
    if isinstance(clip_value, bool) or not isinstance(clip_value, (int, float)) or not math.isfinite(clip_value):
        raise ValueError(who + "clip_value must be a finite float, got %r" % (clip_value,))
    if not _is_int(chunk_rows) or not 1 <= chunk_rows <= MAX_CHUNK:
        raise ValueError(who + "chunk_rows must be an int in [1, %d], got %r" % (MAX_CHUNK, chunk_rows))
    if not hasattr(state_dict, "keys") or not hasattr(state_dict, "__getitem__"):
        raise ValueError(who + "state_dict must be a mapping of names to tensors")
    want = expected_shapes(num_stack, num_layer, head_num_layers, n_components, network_dim=network_dim)
    keys = set(state_dict.keys())
    missing, extra = sorted(set(want) - keys), sorted(keys - set(want))
    if missing:
        raise ValueError(who + "missing key(s) %s" % ", ".join(map(repr, missing)))
    if extra:
        raise ValueError(who + "unexpected key(s) %s" % ", ".join(map(repr, extra)))
    for name, shape in want.items():
        t = state_dict[name]
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape:
            raise ValueError(who + "%s must be a tensor of shape %s, got %s"
                             % (name, shape, tuple(t.shape) if isinstance(t, torch.Tensor) else type(t)))
        if t.dtype != torch.float32:
            raise ValueError(who + "%s must be float32, got %s" % (name, t.dtype))
        if not t.is_contiguous():
            raise ValueError(who + "%s must be contiguous" % name)
    return want


def _acc_row(r, h):
    return (r & 3) + 8 * (r >> 2) + 4 * h


def pack_index(num_stack, num_layer, head_num_layers, n_components, *, network_dim=DIM):
    """The layout of `gd_bc_policy.blob` as an index: blob = flat[pack_index], where flat is the state dict's tensors flattened
    and concatenated in `expected_shapes` order, followed by one zero (the index of every padding element: the odd last
    column of a first embedder layer).  Every parameter lands exactly once.  int64 numpy.
    Forms, with lane = 0..63, c = lane & 31, h = lane >> 5, acc(r, h) = (r & 3) + 8 (r >> 2) + 4 h:
      first  [t 2][s ceil(K / 2)][lane] = W[32 t + c][2 s + h]          (the embedders' first Linear, K = 6 R or 13 R)
      mfma   [t2 2][t 2][r 16][lane]    = W[32 t2 + c][32 t + acc(r, h)]  (every 64 x 64 Linear applied to token tiles)
      trans  [in][out]                  = W[out][in]                      (the Linears of the one-token kernel)
      nat    as stored                                                    (biases, LayerNorm gains and biases)
    At network_dim = 128 (csrc/bc_tile.hpp, BCEnc<4>) the same forms in the same order with T = 4 tiles of 32 features where 64 has 2:
      first  [t 4][s ceil(K / 2)][lane] = W[32 t + c][2 s + h]
      mfma   [t2 4][t 4][r 16][lane]    = W[32 t2 + c][32 t + acc(r, h)]  (every 128 x 128 Linear applied to token tiles)
      trans  [in][out]                  = W[out][in]                      (128 x 128 in the cross layers; head.input_layer is
                                                                           [384][64], the GMM head behind it as at 64)"""
    D, T = network_dim, network_dim // 32
    shapes = expected_shapes(num_stack, num_layer, head_num_layers, n_components, network_dim=D)
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

    def norm(name):
        nat(name + ".weight"), nat(name + ".bias")

    def first(name, k):
        ks = (k + 1) // 2
        t, s = np.arange(T)[:, None, None], np.arange(ks)[None, :, None]
        col = 2 * s + h[None, None, :] + 0 * t
        idx = base[name + ".weight"] + (32 * t + c[None, None, :]) * k + col
        parts.append(np.where(col < k, idx, zero).reshape(-1))
        nat(name + ".bias")

    def mfma(name):
        t2, t, r = np.arange(T)[:, None, None, None], np.arange(T)[None, :, None, None], np.arange(16)[None, None, :, None]
        col = 32 * t + acc[r, h[None, None, None, :]]
        parts.append((base[name + ".weight"] + (32 * t2 + c[None, None, None, :]) * D + col).reshape(-1))
        nat(name + ".bias")

    def trans(name):
        out, inp = shapes[name + ".weight"]
        parts.append((base[name + ".weight"] + np.arange(out)[None, :] * inp + np.arange(inp)[:, None]).reshape(-1))
        nat(name + ".bias")

    for net, k in zip(NETS, NET_K):
        first(net + ".0", k * num_stack)
        norm(net + ".2")
        for i in range(1, 4):
            mfma("%s.%d" % (net, 4 * i))
            norm("%s.%d" % (net, 4 * i + 2))
    for blk, n in zip(SELF_BLOCKS, (num_layer[0], num_layer[1], num_layer[1])):
        for i in range(n):
            p = "%s.%d" % (blk, i)
            norm(p + ".0.module.norm")
            for proj in "qkvo":
                mfma(p + ".0.module.attention.%s_proj" % proj)
            norm(p + ".1.module.0")
            mfma(p + ".1.module.1")
            mfma(p + ".1.module.3")
    for p in CROSS_LAYERS:
        norm(p + ".0.module.q_norm")
        norm(p + ".0.module.kv_norm")
        trans(p + ".0.module.attention.q_proj")
        mfma(p + ".0.module.attention.k_proj")
        mfma(p + ".0.module.attention.v_proj")
        trans(p + ".0.module.attention.o_proj")
        norm(p + ".1.module.0")
        trans(p + ".1.module.1")
        trans(p + ".1.module.3")
    trans("head.input_layer.0")
    for i in range(head_num_layers):
        trans("head.residual_block.%d.0" % i)
    trans("head.head")
    return np.concatenate([np.asarray(p, dtype=np.int64).reshape(-1) for p in parts])


def scratch_floats(max_agents, chunk_rows, network_dim=DIM):
    return chunk_rows * 3 * (max_agents + ROADS) * network_dim


class DeviceBCPolicy:
    NETWORK_DIMS = (DIM, 128)  # the forward is built at both (the backward: bc_train.TrainableBCPolicyDim, the update: bc_opt.DeviceBCDim); the probes at 64 only
    network_dim, context_width = DIM, CONTEXT  # (an instance sets its own)

    def __init__(self, state_dict, max_agents=128, num_stack=5, num_layer=(3, 2), num_head=4, head_num_layers=2,
                 n_components=6, clip_value=-20.0, *, device="cuda", chunk_rows=DEFAULT_CHUNK, **fixed):
        """state_dict: the reference module's, float32.  max_agents: 64 or 128.  num_stack: 1..8.  num_layer: (fusion layers,
        ro_attn / rg_attn layers), 1..4 each.  head_num_layers: 0..4.  n_components: 1..16.  clip_value: a float.  chunk_rows:
        the rows the scratch holds (1..4096).  fixed: network_dim, head_dim, network_num_layers, act_func, dropout, action_dim,
        time_dim, use_tom, accepted only at the values that are built (64 or 128, 64, 4, 'tanh', 0.0, 3, 1, None).  Anything else, a
        missing or extra key, a wrong shape or dtype is a ValueError raised before anything reaches the device."""
        unknown = sorted(set(fixed) - FIXED)
        if unknown:
            raise ValueError(WHO + "unknown argument(s) %s" % ", ".join(unknown))
        num_layer = tuple(num_layer) if isinstance(num_layer, list) else num_layer
        self._cfg = dict(max_agents=max_agents, num_stack=num_stack, num_layer=num_layer, num_head=num_head,
                         head_num_layers=head_num_layers, n_components=n_components, clip_value=clip_value,
                         chunk_rows=chunk_rows, **fixed)
        shapes = check_bc_args(state_dict, network_dims=self.NETWORK_DIMS, **self._cfg)
        self.network_dim = D = fixed.get("network_dim", DIM)
        self.context_width = 3 * D
        try:
            dev = torch.device(device)
        except (RuntimeError, TypeError) as e:
            raise ValueError(WHO + "device: %s" % e)
        if dev.type != "cuda":
            raise ValueError(WHO + "the policy runs on the GPU (there is no host path), got device %r" % (device,))
        self.max_agents, self.num_stack, self.num_layer = max_agents, num_stack, num_layer
        self.head_num_layers, self.n_components, self.clip_value = head_num_layers, n_components, float(clip_value)
        self.chunk_rows = chunk_rows
        self.obs_width = obs_width(max_agents)
        self._L = _capi.lib()
        self.device = dev if dev.index is not None else torch.device("cuda", torch.cuda.current_device())
        self._names = tuple(shapes)
        self._index = torch.from_numpy(pack_index(num_stack, num_layer, head_num_layers, n_components, network_dim=D)).to(self.device)
        self._zero = torch.zeros(1, dtype=torch.float32, device=self.device)
        self.blob = torch.empty(self._index.numel(), dtype=torch.float32, device=self.device)
        self._scratch = torch.empty(scratch_floats(max_agents, chunk_rows, D), dtype=torch.float32, device=self.device)
        self._pack(state_dict)

    @classmethod
    def from_state_dict(cls, state_dict, max_agents=128, num_stack=5, **kw):
        return cls(state_dict, max_agents, num_stack, **kw)

    def _pack(self, sd):
        with torch.no_grad():
            flat = torch.cat([sd[k].detach().to(self.device).reshape(-1) for k in self._names] + [self._zero])
            torch.index_select(flat, 0, self._index, out=self.blob)

    def load_state_dict(self, state_dict):
        """Re-pack after an optimiser step: the same keys, shapes and dtypes (ValueError otherwise).  For tensors already on
        the device this is a concatenation and one gather on the device, on torch's current stream."""
        check_bc_args(state_dict, network_dims=self.NETWORK_DIMS, **self._cfg)
        self._pack(state_dict)

    def nbytes(self, B):
        """What a call of B rows touches beyond its inputs, in bytes: the blob; the scratch, which is sized to the chunk and
        not to B -- chunk_rows * 3 * (A + 200) * network_dim float32 (32.2 MB at the default chunk of 128 rows, A = 128 and
        network_dim 64; 64.5 MB at 128); and every output of the row at once (context, means, covariances and their logs,
        weights, actions, nll, component, ego_attn_score)."""
        C_ = self.n_components
        per_row = 4 * (self.context_width + 3 * 3 * C_ + C_ + 3 + 1 + 1 + HEADS * (self.max_agents - 1))
        return 4 * (int(self.blob.numel()) + int(self._scratch.numel())) + B * per_row

    # ---- argument checks

    def _tensor(self, name, t, dtypes, shape):
        if not isinstance(t, torch.Tensor) or t.dtype not in dtypes or tuple(t.shape) != tuple(shape) or t.device != self.device \
                or not t.is_contiguous():
            raise ValueError(WHO + "%s must be a contiguous %s tensor of shape %s on %s"
                             % (name, " or ".join(str(d) for d in dtypes), tuple(shape), self.device))
        return t

    def _inputs(self, obs, partner_mask, road_mask):
        R, A = self.num_stack, self.max_agents
        if not isinstance(obs, torch.Tensor) or obs.dim() != 3 or tuple(obs.shape[1:]) != (R, self.obs_width):
            raise ValueError(WHO + "obs must be a [B, %d, %d] tensor (num_stack %d, max_agents %d)" % (R, self.obs_width, R, A))
        B = int(obs.shape[0])
        if not 1 <= B <= MAX_ROWS:
            raise ValueError(WHO + "B must be in [1, %d], got %d" % (MAX_ROWS, B))
        self._tensor("obs", obs, (torch.float32,), (B, R, self.obs_width))
        self._tensor("partner_mask", partner_mask, (torch.bool, torch.uint8), (B, R, A - 1))
        self._tensor("road_mask", road_mask, (torch.bool, torch.uint8), (B, R, ROADS))
        return B

    def _expert(self, expert, B):
        if isinstance(expert, torch.Tensor) and tuple(expert.shape) == (B, 1, ACTION_DIM):
            expert = expert.view(B, ACTION_DIM)
        return self._tensor("expert_actions ([B, 1, 3] or [B, 3])", expert, (torch.float32,), (B, ACTION_DIM))

    _OUT_SHAPES = dict(context=lambda s, B: (B, s.context_width), means=lambda s, B: (B, 1, s.n_components, 3),
                       log_covariances=lambda s, B: (B, 1, s.n_components, 3), covariances=lambda s, B: (B, 1, s.n_components, 3),
                       weights=lambda s, B: (B, 1, s.n_components), actions=lambda s, B: (B, 1, 3), nll=lambda s, B: (B,),
                       ego_attn_score=lambda s, B: (B, HEADS, s.max_agents - 1), component=lambda s, B: (B,))

    def forward(self, obs, partner_mask, road_mask, want, *, deterministic=True, u=None, z=None, expert_actions=None, out=None,
                rows=None, readout=None):
        """The one C call.  want: the names of the outputs to write, out of context, means, log_covariances, covariances,
        weights, actions, nll, ego_attn_score, component (`_OUT_SHAPES`); out: a dict with tensors for some of them, to be
        overwritten.  Returns a dict of the wanted tensors.  rows: None for all B rows, or a `policy.LiveRows` of this B
        (`policy.live_rows(mask, out=)`): the forward then runs on the listed rows only (`gd_bc_forward_rows`), reads index r of
        every input and writes index r of every output with the bits the full forward gives that row; rows that are not
        listed are not written, so every wanted output must be given in out= and keeps its bytes there.  The list's length
        stays on the device: every chunk is launched, and the workgroups past the list return at once.  readout: a
        `bc_readout.ProbeReadout` of this policy (`read`): its outputs join the result, one more launch per chunk
        (`gd_bc_forward_readout` / `gd_bc_forward_rows_readout`).  Every check happens before the launch."""
        from .policy import LiveRows
        if rows is not None and not isinstance(rows, LiveRows):
            raise ValueError(WHO + "rows must be a LiveRows (policy.live_rows(mask)), got %s" % type(rows).__name__)
        if readout is not None:
            self._only_64("read-outs")
        B = self._inputs(obs, partner_mask, road_mask)
        if rows is not None:
            if rows.n != B:
                raise ValueError(WHO + "rows must be a LiveRows of N = %d, got one of N = %d" % (B, rows.n))
            if rows.rows.device != self.device:
                raise ValueError(WHO + "rows is on %s, the policy on %s" % (rows.rows.device, self.device))
            missing = [name for name in want if (out or {}).get(name) is None]
            if missing:
                raise ValueError(WHO + "rows= needs out= for every wanted output (rows that are not listed keep the caller's "
                                 "bytes), missing: %s" % ", ".join(missing))
        ro = None
        if readout is not None:
            from .bc_readout import ProbeReadout
            if not isinstance(readout, ProbeReadout) or readout.policy is not self:
                raise ValueError(WHO + "readout must be a ProbeReadout of this policy")
            ro, ro_res = readout.bind((B,), out, need_out=rows is not None, who=WHO)
            out = {k: v for k, v in (out or {}).items() if k not in ro_res}
        deterministic = bool(deterministic)
        if not deterministic:
            if u is None or z is None:
                raise ValueError(WHO + "u [B] and z [B, 3] are required unless deterministic=True")
        if u is not None:
            self._tensor("u", u, (torch.float32,), (B,))
        if z is not None:
            self._tensor("z", z, (torch.float32,), (B, ACTION_DIM))
        if "nll" in want:
            if expert_actions is None:
                raise ValueError(WHO + "expert_actions is required for the nll")
        if expert_actions is not None:
            expert_actions = self._expert(expert_actions, B)
        out = dict(out or {})
        res = {}
        o = _capi.GdBCOutputs()
        for name in want:
            if name not in self._OUT_SHAPES:
                raise ValueError(WHO + "unknown output %r" % (name,))
            shape = self._OUT_SHAPES[name](self, B)
            dt = torch.int32 if name == "component" else torch.float32
            if out.get(name) is not None:
                res[name] = self._tensor("out " + name, out[name], (dt,), shape)
            else:
                res[name] = torch.empty(shape, dtype=dt, device=self.device)
        for name, t in res.items():
            setattr(o, name, t.data_ptr())
        # The entry, chosen once: gd_bc_forward[_rows][_readout], or gd_bc_forward[_rows]_dim for the wide policy (the 64-wide
        # policy keeps the entry points it had; gd_bc_*_dim at 64 are those, bit for bit).  The tail follows the name.
        wide = self.network_dim != DIM
        entry = "gd_bc_forward" + ("_rows" if rows is not None else "") + ("_dim" if wide else "_readout" if ro is not None else "")
        p = self.c_struct_dim() if wide else self.c_struct()
        tail = ([] if ro is None else [C.byref(ro)]) + ([] if rows is None else [rows.rows.data_ptr(), rows.count.data_ptr()])
        with torch.cuda.device(self.device):
            stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            _capi.check(getattr(self._L, entry)(C.byref(p), obs.data_ptr(), partner_mask.data_ptr(), road_mask.data_ptr(), B,
                                                int(deterministic), None if u is None else u.data_ptr(),
                                                None if z is None else z.data_ptr(),
                                                None if expert_actions is None else expert_actions.data_ptr(), C.byref(o), *tail,
                                                stream), entry)
        if ro is not None:
            res.update(ro_res)
        return res

    def read(self, obs, partner_mask, road_mask, readout, deterministic=True, u=None, z=None, rows=None, out=None):
        """The forward with the probe read-outs of `readout` (a `bc_readout.ProbeReadout` of this policy) taken on the way: a
        dict with actions [B, 1, 3] -- `__call__`'s bits -- and whichever of other_pred [B, Po, A - 1], ego_pred [B, Pe] and
        ego_pred_prime [B, P] (uint8 classes 0 .. 63) the read-out defines.  One C call: the forward's launches plus one per
        chunk right after the tapped layer, whatever the number of probes; no encoder layer runs twice.  out: a dict with
        tensors of an earlier call.  rows: a `LiveRows` of B: only the listed rows are read and written, in every output
        (out= must then hold them all).  No host synchronisation; with out= no allocation."""
        self._only_64("read")
        if out is not None and not isinstance(out, dict):
            raise ValueError(WHO + "read: out must be a dict of the outputs' tensors")
        return self.forward(obs, partner_mask, road_mask, ("actions",), deterministic=deterministic, u=u, z=z, out=out, rows=rows,
                            readout=readout)

    def c_struct(self):
        """A fresh gd_bc_policy over this object's blob and scratch."""
        p = _capi.GdBCPolicy()
        p.max_agents, p.num_stack, p.fusion_layers, p.branch_layers = self.max_agents, self.num_stack, *self.num_layer
        p.head_layers, p.n_components, p.clip_value, p.chunk_rows = self.head_num_layers, self.n_components, self.clip_value, self.chunk_rows
        p.blob, p.blob_floats = self.blob.data_ptr(), self.blob.numel()
        p.scratch, p.scratch_floats = self._scratch.data_ptr(), self._scratch.numel()
        return p

    def c_struct_dim(self):
        """A fresh gd_bc_policy_dim: `c_struct` with this policy's network_dim beside it (the gd_bc_*_dim entry points)."""
        p = _capi.GdBCPolicyDim()
        p.base, p.network_dim, p.reserved = self.c_struct(), self.network_dim, 0
        return p

    def _only_64(self, what):
        """What reads 64-wide tokens (hidden states, probes, read-outs) refuses a wider policy before the device is touched."""
        if self.network_dim != DIM:
            raise ValueError(WHO + "%s is built at network_dim 64 only, this policy has network_dim %d" % (what, self.network_dim))

    TAPS = {"fusion_attn": _capi.LP_TAP_FUSION, "ro_attn": _capi.LP_TAP_RO}

    def hidden(self, obs, partner_mask, road_mask, tap="fusion_attn", layer=None, out=None):
        """The hidden states a linear probe reads (the reference's forward hooks on `fusion_attn` / `ro_attn`,
        baselines/il/linear_probing.py:68-95): [B, A, 64] float32, tokens 0 .. A - 1 (the ego, then the partners) of the tapped
        block's last_hidden_state.  One C call (`gd_bc_hidden`): per chunk the forward's own kernels run and stop at the tap -- for
        'fusion_attn' no branch layer, no cross attention and no head is launched.  layer: None for the block's last layer, or
        an int i in [0, layers of that block): the kernels stop after layer i of the block (`gd_bc_hidden_layer`), the output the
        reference's hook on the block's child str(i) sees; ('ro_attn', 0) is the one baselines/il/test/intervention.py reads.
        out: that tensor of an earlier call.  No host synchronisation; with out= no allocation."""
        self._only_64("hidden")
        B = self._inputs(obs, partner_mask, road_mask)
        if tap not in self.TAPS:
            raise ValueError(WHO + "tap must be 'fusion_attn' or 'ro_attn', got %r" % (tap,))
        if layer is not None:
            from .bc_readout import check_tap
            layer = check_tap(self, tap, layer, WHO)
        shape = (B, self.max_agents, DIM)
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=self.device)
        else:
            self._tensor("out", out, (torch.float32,), shape)
            if out.data_ptr() % 16:
                raise ValueError(WHO + "out must be 16-byte aligned")
        p = self.c_struct()
        with torch.cuda.device(self.device):
            stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            if layer is None:
                _capi.check(self._L.gd_bc_hidden(C.byref(p), obs.data_ptr(), partner_mask.data_ptr(), road_mask.data_ptr(), B,
                                                 self.TAPS[tap], out.data_ptr(), stream), "gd_bc_hidden")
            else:
                _capi.check(self._L.gd_bc_hidden_layer(C.byref(p), obs.data_ptr(), partner_mask.data_ptr(), road_mask.data_ptr(), B,
                                                       self.TAPS[tap], layer, out.data_ptr(), stream), "gd_bc_hidden_layer")
        return out

    def __call__(self, obs, partner_mask, road_mask, deterministic=False, u=None, z=None, out=None, rows=None):
        """obs [B, R, D] float32, partner_mask [B, R, A - 1] and road_mask [B, R, 200] bool or uint8, as
        `DeviceExpertDataset.batch` writes them.  deterministic: the mean of the first component of maximal weight; otherwise
        u [B] float32 in [0, 1) and z [B, 3] float32 standard normals give the rule's draw.  Returns actions [B, 1, 3]; out: that
        tensor of an earlier call.  rows: a `LiveRows` of B (`forward`): only the listed rows are computed and written, out= is then
        required.  No host synchronisation; with out= no allocation."""
        return self.forward(obs, partner_mask, road_mask, ("actions",), deterministic=deterministic, u=u, z=z,
                            out=None if out is None else {"actions": out}, rows=rows)["actions"]

    def context(self, obs, partner_mask, road_mask, out=None, ego_attn_score=None, rows=None):
        """get_context's first value, [B, 3 * network_dim] = [ego | ego_ro | ego_rg]; ego_attn_score: a [B, 4, A - 1] float32 tensor to
        receive its second value.  rows: as in `forward` (out= is then required)."""
        want, o = ["context"], {"context": out}
        if ego_attn_score is not None:
            want.append("ego_attn_score")
            o["ego_attn_score"] = ego_attn_score
        return self.forward(obs, partner_mask, road_mask, want, out=o, rows=rows)["context"]

    def gmm_params(self, obs, partner_mask, road_mask, out=None, rows=None):
        """(means [B, 1, C, 3], covariances [B, 1, C, 3], weights [B, 1, C]) as GMM.get_gmm_params returns them.  rows: as in
        `forward` (out= is then required)."""
        names = ("means", "covariances", "weights")
        if out is not None and (not isinstance(out, (tuple, list)) or len(out) != 3):
            raise ValueError(WHO + "out must be the three tensors (means, covariances, weights)")
        r = self.forward(obs, partner_mask, road_mask, names, out=None if out is None else dict(zip(names, out)), rows=rows)
        return tuple(r[k] for k in names)

    def nll(self, obs, partner_mask, road_mask, expert_actions, out=None, rows=None):
        """gmm_loss's detached per-row value for expert_actions [B, 1, 3] (or [B, 3]): [B] float32.  rows: as in `forward`
        (out= is then required)."""
        return self.forward(obs, partner_mask, road_mask, ("nll",), expert_actions=expert_actions,
                            out=None if out is None else {"nll": out}, rows=rows)["nll"]

    def evaluate(self, ds, batch_size=512):
        """The reference's evaluate() (baselines/il/il.py:99-180): its eight numbers as a dict (`EVAL_NAMES`; tom_loss is 0.0,
        there is no aux head).  ds: a `DeviceExpertDataset` (its batches of batch_size in index order), or an iterable of
        (obs, expert, partner_mask, road_mask, data_idx) batches.  Per batch: one forward and one accumulation launch; the
        sums stay on the device, in batch order with one fixed summation order, and are read ONCE at the end.  The averaging
        is the reference's: per-batch means averaged over batches (a short last batch weighs as much as a full one); the
        std2 figures are global sums over global counts (nan where no row qualifies, as 0 / 0 is there)."""
        if hasattr(ds, "batches"):
            if not _is_int(batch_size) or batch_size < 1:
                raise ValueError(WHO + "evaluate: batch_size must be a positive int, got %r" % (batch_size,))
            batches = ds.batches(batch_size, shuffle=False)
        else:
            batches = ds
        acc = torch.zeros(11, dtype=torch.float32, device=self.device)
        bufs = {}
        for batch in batches:
            obs, expert, pm, rm = batch[:4]
            B = int(obs.shape[0])
            if B not in bufs:
                bufs[B] = dict(actions=torch.empty((B, 1, 3), dtype=torch.float32, device=self.device),
                               nll=torch.empty((B,), dtype=torch.float32, device=self.device))
            r = self.forward(obs, pm, rm, ("actions", "nll"), deterministic=True, expert_actions=expert, out=bufs[B])
            with torch.cuda.device(self.device):
                stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
                _capi.check(self._L.gd_bc_eval_accumulate(B, r["nll"].data_ptr(), r["actions"].data_ptr(),
                                                          self._expert(expert, B).data_ptr(), acc.data_ptr(), stream),
                            "gd_bc_eval_accumulate")
        a = acc.cpu().numpy().astype(np.float64)  # the one host read
        n = a[10]
        with np.errstate(divide="ignore", invalid="ignore"):
            vals = [a[0] / n, a[1] / n, a[2] / n, a[3] / n, a[4] / a[7], a[5] / a[8], a[6] / a[9], 0.0]
        return dict(zip(EVAL_NAMES, (float(v) for v in vals)))
