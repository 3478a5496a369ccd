"""Probe read-outs inside the BC forward: what the reference's closed-loop interpretability scripts read per step.

`ProbeReadout` names a tapped self-attention layer of a `DeviceBCPolicy` and up to 8 + 8 trained `DeviceLinearProbe` heads, and
is what `DeviceBCPolicy.read(...)` and `ClosedLoopBC.run(readout=...)` take.  It is baselines/il/test/intervention.py:140-163:
for pairs of probes, `other_pred` (the position class of every partner token), `ego_pred` (the class of the ego token) and
`ego_pred_prime` (the ego class after row `label` of the other-probe's `head.weight` is added to the ego token).  The reference
collects them with forward hooks and one `predict` per head per step; here ONE launch per chunk (`k_bc_readout`,
csrc/bc_readout.hip) reads the tapped tokens where the forward's attention kernel left them, between two of the forward's own
launches, and the forward goes on: nothing is encoded twice, and the launch count does not depend on the number of probes.  The
rule is csrc/bc_readout_rule.hpp.

    ro = ProbeReadout(bc.policy, tap="ro_attn", layer=0, other=[probe_o1, probe_o10], ego=[probe_e1, probe_e10], labels=10)
    r = bc.policy.read(obs, pm, rm, ro)       # actions [B, 1, 3] (bc(...)'s bits), other_pred [B, 2, A - 1], ego_pred [B, 2],
                                              # ego_pred_prime [B, 2]: uint8 classes 0 .. 63
    ep = loop.run(attention=True, readout=ro) # ClosedLoopBC: the same per step, [91, N, ...], see bc_rollout
    ro.bad_labels                             # [1] int32 on the device: rows read whose label was outside 0 .. 63, summed over
                                              # every call and step since it was last zeroed (ro.bad_labels.zero_())

`('ro_attn', 0)` is the layer the reference script hooks (`bc_policy.ro_attn`'s child '0').  A probe's own `model` does not bind
the tap: the reference applies heads trained on one layer to another.  Where the tap is a probe's own ('fusion_attn' / None
for 'early_lp', 'ro_attn' / None for 'late_lp'), `other_pred` / `ego_pred` are `probe.predict`'s values bit for bit.  The probes'
`packed` and `flat` buffers are taken by pointer at call time, so a probe that trains between two calls is followed in place.

Not here: steering the action with the modified token (the reference only reads `ego_pred_prime`; the action is unchanged here
too), `lp_weight.py`, the plots."""
import torch

from . import _capi
from . import bc_policy as BP

WHO = "ProbeReadout: "
MAX_PROBES = _capi.BC_READOUT_MAX
NO_CLASS = _capi.BC_READOUT_NO_CLASS
OUTPUTS = ("other_pred", "ego_pred", "ego_pred_prime")


def tap_layers(policy, tap):
    """The self-attention layers of the tapped block."""
    return policy.num_layer[0] if tap == "fusion_attn" else policy.num_layer[1]


def check_tap(policy, tap, layer, who=WHO):
    """(tap, layer) of `policy`, refused on the host (ValueError); returns the layer as an int (None: the block's last)."""
    if tap not in BP.DeviceBCPolicy.TAPS:
        raise ValueError(who + "tap must be 'fusion_attn' or 'ro_attn', got %r" % (tap,))
    n = tap_layers(policy, tap)
    if layer is None:
        return n - 1
    if not BP._is_int(layer) or not 0 <= layer < n:
        raise ValueError(who + "layer must be None or an int in [0, %d) for tap %r, got %r" % (n, tap, layer))
    return layer


class ProbeReadout:
    def __init__(self, policy, tap="ro_attn", layer=None, other=(), ego=(), labels=None):
        """policy: the `DeviceBCPolicy` that is read.  tap, layer: the self-attention layer whose output the probes read
        (`DeviceBCPolicy.hidden`'s; None: the block's last).  other / ego: lists of 0 to 8 `DeviceLinearProbe` of exp 'other' /
        'ego', at least one in total, each probing this same policy object with in_features 64 ('early_lp' or 'late_lp').
        labels: None (no intervention), an int (every row's label) or an int64 tensor [N] on the policy's device (row n's
        label); then len(other) == len(ego) and pair p is (ego[p], other[p]).  A label outside 0 .. 63 is no intervention for
        that row and is counted in `bad_labels`.  Everything refused is a ValueError raised before anything reaches the device."""
        from .lp_probe import DeviceLinearProbe
        if not isinstance(policy, BP.DeviceBCPolicy):
            raise ValueError(WHO + "policy must be a DeviceBCPolicy, got %s" % type(policy).__name__)
        if policy.network_dim != 64:
            raise ValueError(WHO + "the read-outs read 64-wide tokens: the policy's network_dim must be 64, got %d" % policy.network_dim)
        self.layer = check_tap(policy, tap, layer)
        lists = []
        for name, probes in (("other", other), ("ego", ego)):
            if not isinstance(probes, (list, tuple)):
                raise ValueError(WHO + "%s must be a list of DeviceLinearProbe, got %s" % (name, type(probes).__name__))
            if len(probes) > MAX_PROBES:
                raise ValueError(WHO + "%s holds %d probes, at most %d are read in one launch" % (name, len(probes), MAX_PROBES))
            for i, pr in enumerate(probes):
                at = "%s[%d]" % (name, i)
                if not isinstance(pr, DeviceLinearProbe):
                    raise ValueError(WHO + "%s must be a DeviceLinearProbe, got %s" % (at, type(pr).__name__))
                if pr.exp != name:
                    raise ValueError(WHO + "%s has exp %r, the list is the %r probes'" % (at, pr.exp, name))
                if pr.policy is not policy:
                    raise ValueError(WHO + "%s probes another policy object (model %r)" % (at, pr.model))
                if pr.in_features != BP.DIM:
                    raise ValueError(WHO + "%s has in_features %d: only probes of the encoder's 64 features are read" % (at, pr.in_features))
            lists.append(tuple(probes))
        self.other, self.ego = lists
        if not self.other and not self.ego:
            raise ValueError(WHO + "at least one probe is required")
        self.policy, self.tap = policy, tap
        self.intervene = labels is not None
        self.label, self.labels, self.bad_labels = 0, None, None
        if self.intervene:
            if len(self.other) != len(self.ego):
                raise ValueError(WHO + "labels needs len(other) == len(ego) (pair p is (ego[p], other[p])), got %d and %d"
                                 % (len(self.other), len(self.ego)))
            if BP._is_int(labels):
                self.label = labels
            elif isinstance(labels, torch.Tensor):
                if labels.dtype != torch.int64 or labels.dim() != 1 or not labels.is_contiguous() or labels.device != policy.device \
                        or labels.data_ptr() % 8:
                    raise ValueError(WHO + "labels must be a contiguous 8-byte aligned int64 tensor [N] on %s" % (policy.device,))
                self.labels = labels
            else:
                raise ValueError(WHO + "labels must be None, an int or an int64 tensor [N], got %s" % type(labels).__name__)
            self.bad_labels = torch.zeros(1, dtype=torch.int32, device=policy.device)

    @property
    def names(self):
        """The outputs this read-out defines, out of other_pred, ego_pred, ego_pred_prime."""
        return tuple(n for n, on in zip(OUTPUTS, (self.other, self.ego, self.intervene)) if on)

    def row_shape(self, name):
        """The shape of one row of output `name`."""
        A = self.policy.max_agents
        return {"other_pred": (len(self.other), A - 1), "ego_pred": (len(self.ego),), "ego_pred_prime": (len(self.ego),)}[name]

    def row_nbytes(self):
        """Bytes one row of all outputs takes (one byte per class)."""
        n = 0
        for name in self.names:
            k = 1
            for v in self.row_shape(name):
                k *= v
            n += k
        return n

    def bind(self, lead, out, need_out=False, who=WHO):
        """The gd_bc_readout of a call whose outputs have the leading dimensions `lead` ((B,) or (91, N)): out's tensors are
        checked, missing ones made (refused with need_out).  Returns (struct, dict of the output tensors)."""
        pol, rows = self.policy, lead[-1]
        if self.labels is not None and int(self.labels.shape[0]) != rows:
            raise ValueError(who + "labels has %d entries, the call %d rows" % (int(self.labels.shape[0]), rows))
        r = _capi.GdBCReadout()
        r.tap, r.layer, r.n_other, r.n_ego = pol.TAPS[self.tap], self.layer, len(self.other), len(self.ego)
        r.intervene = int(self.intervene)
        for dst, probes in ((r.other, self.other), (r.ego, self.ego)):
            for i, pr in enumerate(probes):
                dst[i].packed, dst[i].weight = pr.packed.data_ptr(), pr.flat.data_ptr()
        if self.intervene:
            r.labels = None if self.labels is None else self.labels.data_ptr()
            r.label, r.bad_labels = self.label, self.bad_labels.data_ptr()
        res = {}
        for name in self.names:
            shape = tuple(lead) + self.row_shape(name)
            t = (out or {}).get(name)
            if t is None:
                if need_out:
                    raise ValueError(who + "rows= needs out= for every output (rows that are not listed keep the caller's bytes), "
                                     "missing: %s" % name)
                t = torch.empty(shape, dtype=torch.uint8, device=pol.device)
            elif not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or tuple(t.shape) != shape or t.device != pol.device \
                    or not t.is_contiguous():
                raise ValueError(who + "out %s must be a contiguous uint8 tensor of shape %s on %s" % (name, shape, pol.device))
            res[name] = t
            setattr(r, name, t.data_ptr())
            stride = 1
            for v in self.row_shape(name):
                stride *= v
            setattr(r, {"other_pred": "other_stride", "ego_pred": "ego_stride", "ego_pred_prime": "prime_stride"}[name], stride)
        return r, res
