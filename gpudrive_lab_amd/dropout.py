"""Training-mode dropout of the device policy: the mask rule and its device call counter.

The reference's PPO baseline trains with `network.dropout: 0.01` and never calls `.eval()`, so the four `nn.Dropout` layers
of `late_fusion.NeuralNet` -- after the tanh of each of the three embedders and after `shared_embed`'s linear -- are live in
the rollout forward and in the training forward and backward.  torch's random stream cannot be reproduced, so the masks here
are this project's rule (csrc/dropout_rule.hpp, stated there in full): whether an element is kept is a pure function of
(seed, call, row, site, entity, feature) through Philox4x32-10 cut into 16-bit fields.  An element is dropped iff its field is
below `threshold = floor(p * 65536)`; a kept element is multiplied by `scale = 1 / (1 - p)` in float32, as torch does.

    rule = DropoutRule(0.01, seed=7)
    ppo = DevicePPO(net.state_dict(), max_agents=128, ego_width=6, dropout_rule=rule)   # ppo.policy shares the rule
    pol = DevicePolicy.from_state_dict(sd, dropout_rule=rule)                           # or on its own; pol.eval() unmasks

`call` counts the masked forward / evaluate calls.  It lives on the device: every kernel of a call reads it and the call's
last launch advances it, so a loop of calls needs no host value that changes and can be captured in a graph.  Objects that
share a rule draw from ONE stream of call indices and must therefore run on one CUDA stream (or be ordered by events).

The effective drop probability is threshold / 65536 (p rounded down to a multiple of 2^-16)."""
import numpy as np
import torch

from . import _capi

FIELD_BITS = 16
MIN_P = 2.0 ** -FIELD_BITS


def check_rule_args(p, seed):
    """What `DropoutRule` refuses of p and seed (ValueError, on the host).  Returns (p, seed, threshold, scale)."""
    who = "DropoutRule: "
    if isinstance(p, bool) or not isinstance(p, (int, float)) or not MIN_P <= p < 1.0:
        raise ValueError(who + "p must be a number in [2^-16, 1), got %r" % (p,))
    if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 2 ** 64:
        raise ValueError(who + "seed must be an int in [0, 2^64), got %r" % (seed,))
    p = float(p)
    threshold = int(np.floor(p * 65536.0))
    if not 1 <= threshold <= 65535 or not np.float32(p) < np.float32(1.0):
        raise ValueError(who + "p = %r leaves no element to keep (p rounds to 1)" % (p,))
    scale = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))
    return p, seed, threshold, scale


def check_rule(rule, who, device=None):
    """`dropout_rule=` of DevicePolicy, TrainablePolicy and DevicePPO: None or a DropoutRule (on `device`, when given)."""
    if rule is None:
        return None
    if not isinstance(rule, DropoutRule):
        raise ValueError(who + "dropout_rule must be a DropoutRule or None, got %r" % (type(rule).__name__,))
    if device is not None and rule.device != device:
        raise ValueError(who + "dropout_rule lives on %s, the object on %s" % (rule.device, device))
    return rule


class DropoutRule:
    def __init__(self, p, seed, device="cuda"):
        """p: the drop probability, in [2^-16, 1).  seed: an int in [0, 2^64).  Owns the device call counter (and one scratch
        word), allocated here; refusals are ValueError raised on the host before anything reaches the device."""
        self.p, self.seed, self.threshold, self.scale = check_rule_args(p, seed)
        try:
            dev = torch.device(device)
        except (RuntimeError, TypeError) as e:
            raise ValueError("DropoutRule: device: %s" % e)
        if dev.type != "cuda":
            raise ValueError("DropoutRule: the masks are drawn on the GPU (there is no host path), got device %r" % (device,))
        self.device = dev if dev.index is not None else torch.device("cuda", torch.cuda.current_device())
        # [0]: the index the next masked call consumes; [1]: the word gd_dropout.used points to when the caller has none
        self._state = torch.zeros(2, dtype=torch.int64, device=self.device)

    @property
    def call(self):
        """The index the next masked forward / evaluate consumes (one host read)."""
        return int(self._state[0].item()) & (2 ** 64 - 1)

    def seek(self, k):
        """Set the index the next masked call consumes (a fill on torch's current stream)."""
        if isinstance(k, bool) or not isinstance(k, int) or not 0 <= k < 2 ** 64:
            raise ValueError("DropoutRule.seek: an int in [0, 2^64), got %r" % (k,))
        self._state[0:1].fill_(k if k < 2 ** 63 else k - 2 ** 64)

    @property
    def nbytes(self):
        return self._state.numel() * self._state.element_size()

    def struct(self, used=None):
        """The gd_dropout of this rule; used: an int64 tensor of one element that receives the index evaluate consumes (the
        rule's own scratch word when None)."""
        d = _capi.GdDropout()
        d.seed, d.threshold, d.scale = self.seed, self.threshold, self.scale
        d.call = self._state.data_ptr()
        d.used = self._state.data_ptr() + 8 if used is None else used.data_ptr()
        return d
