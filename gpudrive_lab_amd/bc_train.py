"""The device BC policy as a differentiable torch module: the training step of the reference's imitation learning
(baselines/il/il.py:248-292) with the forward, the GMM loss and the backward to every parameter in HIP.

    tbp = TrainableBCPolicy.from_state_dict(net.state_dict(), max_agents=128, num_stack=5, num_layer=(3, 2), num_head=4,
                                            head_num_layers=2, n_components=6, clip_value=-20.0)
    opt = torch.optim.AdamW(tbp.parameters(), lr=5e-4, eps=1e-4)
    obs, expert, pm, rm, data_idx = ds.batch(sel)                 # DeviceExpertDataset, unchanged
    loss = tbp(obs, pm, rm, expert).mean()                        # gmm_loss(...)[0]
    opt.zero_grad(); loss.backward(); torch.nn.utils.clip_grad_norm_(tbp.parameters(), 20); opt.step()
    bc.load_state_dict(tbp.state_dict())                          # a DeviceBCPolicy follows
(`bc_opt.DeviceBC` is these four lines as one C call, with the evaluation policy following in place.)

`tbp(...)` is `DeviceBCPolicy.nll` bit for bit on the same weights (the same C call).  Its backward is one more C call,
`gd_bc_backward` (csrc/bc_grad.hip): per chunk of `chunk_rows` rows it runs the forward again with the forward's own kernels,
keeps the self-attention layers' inputs in chunk-sized scratch and walks the layers backwards, rebuilding the scores per
32 x 32 tile.  Nothing is saved between forward and backward but the caller's own tensors and the packed weights, and no
tensor with an L x L extent exists.  Memory does not depend on B (`nbytes`).  No atomics: equal inputs, `chunk_rows` and
`partials` give equal bits.

The parameters carry the reference module's names and shapes (`bc_policy.expected_shapes`), so `state_dict()` loads into and
from the reference `EarlyFusionAttnBCNet`, and any torch optimiser works.  The gradients are autograd's of the reference: a
masked score receives none (a row whose keys are all masked gives its uniform share to the values and nothing to queries
and keys), the covariance clamp passes the gradient on [clip_value, 3.58352], bounds included, and an exact 0 outside, the
head's ReLU passes nothing at a pre-activation <= 0.  `obs` gets no gradient.

`TrainableBCPolicyDim` is the same module at the widths the backward is built at, 64 and 128: `network_dim=128` (with head_dim 64,
num_layer (4, 3): the model of the reference's sweep, baselines/il/sweep.yaml) trains on the kernels' T = 4 instantiations through
`gd_bc_forward_dim` / `gd_bc_backward_dim`, and a `DeviceBCPolicy(..., network_dim=128)` follows with `load_state_dict`.
`TrainableBCPolicy` itself keeps refusing any width but 64, as `gd_bc_backward` keeps taking a `gd_bc_policy`.

Not here: gradient clipping and AdamW (any torch optimiser works on this module; `bc_opt.DeviceBC` is the whole step on the
device, gd_bc_update, without it); non-zero dropout; `aux_head` / `use_tom`; `l1_loss` / `focal_loss`; bf16; a gradient with respect to the
observations; any tuning beyond one wave per workgroup.  (The whole step on the device at 128 is `bc_opt.DeviceBCDim`.)"""
import ctypes as C

import numpy as np
import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import _capi
from . import bc_policy as BP

WHO = "TrainableBCPolicy: "
DEFAULT_PARTIALS = 128
MAX_PARTIALS = 4096
_ALLOCATIONS = 16  # tensors a step allocates, for the allocator's rounding in nbytes


def grad_floats(num_stack, num_layer, head_num_layers, n_components, *, network_dim=BP.DIM):
    return sum(int(np.prod(s)) for s in BP.expected_shapes(num_stack, num_layer, head_num_layers, n_components,
                                                           network_dim=network_dim).values())


def grad_scratch_floats(max_agents, chunk_rows, num_layer, blob_floats, *, network_dim=BP.DIM):
    """gd_bc_grad.scratch: the transposed weights, the self-attention layers' inputs, and five token buffers with the
    softmax row statistics of one chunk (csrc/bc_grad.hip `bc_grad_scratch_floats` is the C side's one statement of it)."""
    return (blob_floats + 63) // 64 * 64 + chunk_rows * (max_agents + BP.ROADS) * (network_dim * (num_layer[0] + num_layer[1] + 5) + 16)


class _BCStep(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mod, obs, partner_mask, road_mask, expert, *params):
        B, dev = int(obs.shape[0]), obs.device
        with torch.no_grad():
            flat = torch.cat([p.reshape(-1) for p in params] + [mod._zero])
            blob = torch.index_select(flat, 0, mod._index)
        nll = torch.empty(B, dtype=torch.float32, device=dev)
        o = _capi.GdBCOutputs()
        o.nll = nll.data_ptr()
        p = mod._policy_struct(blob)
        forward, who = (_capi.lib().gd_bc_forward_dim, "gd_bc_forward_dim") if mod._wide else (_capi.lib().gd_bc_forward, "gd_bc_forward")
        with torch.cuda.device(dev):
            stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            _capi.check(forward(C.byref(p), obs.data_ptr(), partner_mask.data_ptr(), road_mask.data_ptr(), B, 1,
                                None, None, expert.data_ptr(), C.byref(o), stream), who)
        ctx.save_for_backward(obs, partner_mask, road_mask, expert, *params)  # (torch's version check catches a step in between)
        ctx.mod, ctx.blob = mod, blob
        return nll

    @staticmethod
    @once_differentiable
    def backward(ctx, d_nll):
        obs, partner_mask, road_mask, expert = ctx.saved_tensors[:4]
        mod, blob = ctx.mod, ctx.blob
        B, dev = int(obs.shape[0]), obs.device
        d_nll = d_nll.to(torch.float32).contiguous()
        grad = torch.empty(mod._G, dtype=torch.float32, device=dev)
        p, g = mod._policy_struct(blob), _capi.GdBCGrad()
        g.scratch, g.scratch_floats = mod._grad_scratch.data_ptr(), mod._grad_scratch.numel()
        g.partials, g.grad_floats, g.num_partials = mod._partials.data_ptr(), mod._G, mod.partials
        backward, who = (_capi.lib().gd_bc_backward_dim, "gd_bc_backward_dim") if mod._wide else (_capi.lib().gd_bc_backward, "gd_bc_backward")
        with torch.cuda.device(dev):
            stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            _capi.check(backward(C.byref(p), C.byref(g), obs.data_ptr(), partner_mask.data_ptr(), road_mask.data_ptr(), B,
                                 expert.data_ptr(), d_nll.data_ptr(), None, grad.data_ptr(), stream), who)
        views, o = [], 0
        for shape in mod._shapes:
            k = int(np.prod(shape))
            views.append(grad[o:o + k].view(shape))
            o += k
        return (None, None, None, None, None) + tuple(views)


class TrainableBCPolicy(nn.Module):
    NETWORK_DIMS = (BP.DIM,)  # the widths this name accepts; `TrainableBCPolicyDim` is the class at every width that is built

    def __init__(self, state_dict, max_agents=128, num_stack=5, num_layer=(3, 2), num_head=4, head_num_layers=2,
                 n_components=6, clip_value=-20.0, *, device=None, chunk_rows=BP.DEFAULT_CHUNK, partials=None, **fixed):
        """`DeviceBCPolicy`'s arguments, refused alike on the host (ValueError) before anything reaches the device.  device:
        where the parameters go (None: where the state dict's tensors are); as with any module they may sit on the host, for
        a state dict to be exchanged -- `forward` is what needs the GPU and says so.  partials: P in [1, 4096], the number
        of one-wave workgroups of each backward launch and of partial gradients the last launch adds in order (default 128:
        128 times the parameters, about 150 MB, allocated at the first forward and kept).  The sums are deterministic for a
        given P and chunk_rows.  fixed: `DeviceBCPolicy`'s; network_dim must be one of the class's NETWORK_DIMS."""
        super().__init__()
        unknown = sorted(set(fixed) - BP.FIXED)
        if unknown:
            raise ValueError(WHO + "unknown argument(s) %s" % ", ".join(unknown))
        num_layer = tuple(num_layer) if isinstance(num_layer, list) else num_layer
        shapes = BP.check_bc_args(state_dict, max_agents=max_agents, num_stack=num_stack, num_layer=num_layer, num_head=num_head,
                                  head_num_layers=head_num_layers, n_components=n_components, clip_value=clip_value,
                                  chunk_rows=chunk_rows, who=WHO, network_dims=self.NETWORK_DIMS, **fixed)
        self.network_dim = D = fixed.get("network_dim", BP.DIM)
        self._wide = D != BP.DIM  # a 64-wide instance of either class calls gd_bc_forward / gd_bc_backward
        if partials is None:
            partials = DEFAULT_PARTIALS
        if not BP._is_int(partials) or not 1 <= partials <= MAX_PARTIALS:
            raise ValueError(WHO + "partials must be an int in [1, %d], got %r" % (MAX_PARTIALS, partials))
        dev = None
        if device is not None:
            try:
                dev = torch.device(device)
            except (RuntimeError, TypeError) as e:
                raise ValueError(WHO + "device: %s" % e)
        self.max_agents, self.num_stack, self.num_layer = max_agents, num_stack, num_layer
        self.head_num_layers, self.n_components, self.clip_value = head_num_layers, n_components, float(clip_value)
        self.chunk_rows, self.partials = chunk_rows, partials
        self.obs_width = BP.obs_width(max_agents)
        self._names, self._shapes = tuple(shapes), tuple(shapes.values())
        self._G = grad_floats(num_stack, num_layer, head_num_layers, n_components, network_dim=D)
        for name in self._names:  # e.g. fusion_attn.0.0.module.norm.weight: plain containers under the reference's names
            *path, leaf = name.split(".")
            at = self
            for part in path:
                if part not in at._modules:
                    at.add_module(part, nn.Module())
                at = at._modules[part]
            at.register_parameter(leaf, nn.Parameter(state_dict[name].detach().to(device=dev, copy=True)))
        index = BP.pack_index(num_stack, num_layer, head_num_layers, n_components, network_dim=D)
        self.register_buffer("_index", torch.from_numpy(index).to(dev), persistent=False)
        self.register_buffer("_zero", torch.zeros(1, dtype=torch.float32, device=dev), persistent=False)
        self._sizes = (BP.scratch_floats(max_agents, chunk_rows, D),
                       grad_scratch_floats(max_agents, chunk_rows, num_layer, int(index.size), network_dim=D), partials * self._G)
        self._scratch = self._grad_scratch = self._partials = None

    def _workspace(self, dev):
        """The forward's scratch, the backward's and the partial sums: allocated at the first forward, kept, sized to the chunk."""
        if self._scratch is None or self._scratch.device != dev:
            self._scratch, self._grad_scratch, self._partials = (torch.empty(n, dtype=torch.float32, device=dev) for n in self._sizes)

    @classmethod
    def from_state_dict(cls, state_dict, max_agents=128, num_stack=5, **kw):
        return cls(state_dict, max_agents, num_stack, **kw)

    def _policy_struct(self, blob):
        """A fresh gd_bc_policy, or at 128 the gd_bc_policy_dim that holds it (what the entries of `_BCStep` take)."""
        if self._wide:
            pd = _capi.GdBCPolicyDim()
            pd.network_dim, pd.reserved = self.network_dim, 0
            p = pd.base
        else:
            pd = p = _capi.GdBCPolicy()
        p.max_agents, p.num_stack, p.fusion_layers, p.branch_layers = self.max_agents, self.num_stack, *self.num_layer
        p.head_layers, p.n_components, p.clip_value, p.chunk_rows = self.head_num_layers, self.n_components, self.clip_value, self.chunk_rows
        p.blob, p.blob_floats = blob.data_ptr(), blob.numel()
        p.scratch, p.scratch_floats = self._scratch.data_ptr(), self._scratch.numel()
        return pd

    def nbytes(self, B):
        """An upper bound on everything a step (forward plus backward) of B rows touches beyond its inputs, in bytes.  The
        part that does not depend on B: the flat weights and the blob of the step, the flat gradient and the `.grad`
        tensors of a first backward, the allocator's rounding; and what the module allocates at its first forward: the forward's scratch
        (chunk_rows * 3 * (A + 200) * network_dim floats), the backward's (the transposed weights and chunk_rows * (A + 200) *
        (network_dim * (layers + 5) + 16) floats) and `partials` times the parameters.  Per row: the nll, its upstream gradient
        and that gradient's contiguous float32 copy.  At the reference sweep's model (network_dim 128, num_layer (4, 3), num_stack 5,
        6 components) the parameters are 1,399,274 floats and the default 128 partials 716 MB: pass a smaller `partials` where
        that is too much."""
        G = self._G
        fixed = 4 * ((G + 1) + int(self._index.numel()) + 2 * G) + 512 * _ALLOCATIONS
        once = 4 * sum(self._sizes) + 512 * 3
        return fixed + once + 12 * B

    def forward(self, obs, partner_mask, road_mask, expert_actions):
        """obs [B, R, D] float32, partner_mask [B, R, A - 1] and road_mask [B, R, 200] bool or uint8, expert_actions [B, 1, 3] or
        [B, 3] float32, contiguous, on the parameters' GPU, as `DeviceExpertDataset.batch` writes them.  Returns nll [B]
        float32 (gmm_loss's per-row value), differentiable with respect to the parameters (once).  One C call here and one in
        the backward, on torch's current stream; no host synchronisation."""
        R, A = self.num_stack, self.max_agents
        if not isinstance(obs, torch.Tensor) or obs.dim() != 3 or tuple(obs.shape[1:]) != (R, self.obs_width):
            raise ValueError(WHO + "obs must be a [B, %d, %d] tensor (num_stack %d, max_agents %d)" % (R, self.obs_width, R, A))
        if obs.requires_grad:
            raise ValueError(WHO + "obs must not require grad (there is no gradient with respect to the observations)")
        B, dev = int(obs.shape[0]), obs.device
        if not 1 <= B <= BP.MAX_ROWS:
            raise ValueError(WHO + "B must be in [1, %d], got %d" % (BP.MAX_ROWS, B))
        if dev.type != "cuda":
            raise ValueError(WHO + "obs must be on the GPU (there is no host path), got %s" % (dev,))
        if isinstance(expert_actions, torch.Tensor) and tuple(expert_actions.shape) == (B, 1, BP.ACTION_DIM):
            expert_actions = expert_actions.view(B, BP.ACTION_DIM)
        for name, t, dtypes, shape in (("obs", obs, (torch.float32,), (B, R, self.obs_width)),
                                       ("partner_mask", partner_mask, (torch.bool, torch.uint8), (B, R, A - 1)),
                                       ("road_mask", road_mask, (torch.bool, torch.uint8), (B, R, BP.ROADS)),
                                       ("expert_actions ([B, 1, 3] or [B, 3])", expert_actions, (torch.float32,), (B, BP.ACTION_DIM))):
            if not isinstance(t, torch.Tensor) or t.dtype not in dtypes or tuple(t.shape) != shape or t.device != dev \
                    or not t.is_contiguous() or t.requires_grad:
                raise ValueError(WHO + "%s must be a contiguous %s tensor of shape %s on %s that does not require grad"
                                 % (name, " or ".join(str(d) for d in dtypes), shape, dev))
        params = []
        for name, shape in zip(self._names, self._shapes):
            p = self.get_parameter(name)
            if p.device != dev or p.dtype != torch.float32 or tuple(p.shape) != shape or not p.is_contiguous():
                raise ValueError(WHO + "parameter %s must be a contiguous float32 tensor of shape %s on %s" % (name, shape, dev))
            params.append(p)
        self._workspace(dev)
        return _BCStep.apply(self, obs, partner_mask, road_mask, expert_actions, *params)


class TrainableBCPolicyDim(TrainableBCPolicy):
    """`TrainableBCPolicy` at every width the backward is built at: `network_dim=64` (the default; the same C calls and bits
    as `TrainableBCPolicy`) or `network_dim=128`, the reference sweep's model."""
    NETWORK_DIMS = (BP.DIM, 128)
