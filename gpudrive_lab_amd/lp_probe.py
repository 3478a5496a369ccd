"""The device linear probe: the reference's linear-probing loop on the hidden states of the device BC policy.

`DeviceLinearProbe` is baselines/il/linear_probing.py:97-342 with `LinearProbPosition` (gpudrive/integrations/il/
linear_probing/lp_model.py:48-85) as the head: an `nn.Linear(K, 64)` over the 8 x 8 future-position classes that
`DeviceFutureDataset` labels, trained with mean cross-entropy and `AdamW(lr, eps=1e-4)` on the rows the batch's mask selects,
and scored by accuracy, loss and macro F1 per batch plus the same on the out-of-distribution (OOD) label subset at evaluation.
The rule -- every rounding, the order of every sum -- is csrc/lp_rule.hpp; the kernels are csrc/lp_probe.hip.

    probe = DeviceLinearProbe(bc.policy, {"head.weight": w, "head.bias": b}, model="early_lp", exp="other", lr=0.0015)
    ds = episode.future_dataset(rollout_len=5, pred_len=1, future_step=5, exp="other")
    probe.update(*ds.batch(sel))            # the eight tensors as they are; ONE C call (gd_lp_update)
    probe.fit(ds, total_gradient_steps=10_000, batch_size=256, eval_ds=val, eval_freq=2000, generator=g)
    probe.losses()                          # pos_loss, pos_accuracy, pos_f1_macro, steps, skipped, bad_labels: one host read
    probe.evaluate(val, batch_size=256)     # eval/pos_*, eval/ood_*: one host read
    probe.logits(obs, pm, rm); probe.predict(obs, pm, rm)        # LinearProbPosition.forward / .predict
    probe.state_dict(); probe.best_state_dict(); probe.optimizer_state_dict(); probe.load_optimizer_state_dict(sd)

model: 'early_lp' reads the last layer of `fusion_attn`, 'late_lp' of `ro_attn` (`DeviceBCPolicy.hidden`'s taps; the forward
stops there: for 'early_lp' no branch layer, no cross attention and no head runs), 'baseline' reads obs itself and takes no
policy.  exp: 'ego' probes token 0, 'other' tokens 1 .. A - 1 (A - 1 columns where the reference hard-codes 127); the probe
reads them from the chunk scratch where the attention kernel left them, so no [B, A - 1, 64] tensor exists.  The probe reads
`policy.blob` at call time, so it follows a `DeviceBC` that is still training.

A batch that selects no row is the reference's `continue`: the device leaves the optimiser untouched and counts it in
`skipped`; no host read decides it.  A selected row whose label is outside [0, 63] is dropped and counted in `bad_labels`.

Not here: `LinearProbAction` / `LinearProbAngle`, wandb logging, the sweep files, `lp_weight.py`, Pearson correlations and
plots."""
import ctypes as C

import numpy as np
import torch

from . import _capi
from . import bc_policy as BP
from .bc_opt import _number

WHO = "DeviceLinearProbe: "
MODELS = {"early_lp": _capi.LP_EARLY, "late_lp": _capi.LP_LATE, "baseline": _capi.LP_BASELINE}
EXPS = {"other": _capi.IL_FUTURE_OTHER, "ego": _capi.IL_FUTURE_EGO}
CLASSES = 64
DEFAULT_PARTIALS, MAX_PARTIALS = 128, 4096
KEYS = ("head.weight", "head.bias")
TRAIN_NAMES = ("pos_loss", "pos_accuracy", "pos_f1_macro")
EVAL_NAMES = ("eval/pos_accuracy", "eval/pos_loss", "eval/pos_f1_macro", "eval/ood_accuracy", "eval/ood_loss", "eval/ood_f1_macro")
BEST_LOSS_START = 9999999.0  # linear_probing.py:156


def in_features(model, exp, num_stack):
    """K of the head: 64 on a backbone, 6 R ('ego') or 12 R ('other') for the baseline probe."""
    if model != "baseline":
        return BP.DIM
    return (6 if exp == "ego" else 12) * num_stack


def pack_index(K):
    """The layout of `gd_lp_probe.packed` as an index into [head.weight [64][K] flattened | head.bias | one zero]:
    bc_policy.pack_index's `mfma` form with the columns K .. 63 at the zero, then the bias.  int64 numpy [4160]."""
    lane = np.arange(64)
    c, h = lane & 31, lane >> 5
    acc = np.array([[BP._acc_row(r, hh) for hh in (0, 1)] for r in range(16)])
    t2, t, r = np.arange(2)[:, None, None, None], np.arange(2)[None, :, None, None], np.arange(16)[None, None, :, None]
    col = 32 * t + acc[r, h[None, None, None, :]] + 0 * t2
    idx = (32 * t2 + c[None, None, None, :]) * K + col
    zero = CLASSES * K + CLASSES
    return np.concatenate([np.where(col < K, idx, zero).reshape(-1), CLASSES * K + np.arange(CLASSES)]).astype(np.int64)


def ood_labels(exp):
    """linear_probing.py:137-141."""
    if exp == "other":
        return sorted({x * 8 + y for x in range(8) for y in range(8) if x in (0, 1, 6, 7) or y in (0, 1, 6, 7)})
    return sorted({x * 8 + y for x in range(8) for y in range(8) if x not in (3, 4)})


def macro_f1(tp, n_pred, n_label):
    """sklearn's f1_score(average='macro') from per-class counters: the mean of 2 tp / (pred + label) over the classes that
    occur in either; nan when none does."""
    tp, d = np.asarray(tp, np.float64), np.asarray(n_pred, np.float64) + np.asarray(n_label, np.float64)
    seen = d > 0
    return float((2.0 * tp[seen] / d[seen]).mean()) if seen.any() else float("nan")


def check_probe_args(policy, state_dict, model, exp, lr, eps, betas, weight_decay, partials, max_agents, num_stack):
    """Everything the constructor refuses, on the host (ValueError).  Returns (A, R, K, partials)."""
    if model not in MODELS:
        raise ValueError(WHO + "model must be 'early_lp', 'late_lp' or 'baseline', got %r" % (model,))
    if exp not in EXPS:
        raise ValueError(WHO + "exp must be 'other' or 'ego', got %r" % (exp,))
    if model == "baseline":
        if policy is not None:
            raise ValueError(WHO + "model 'baseline' takes no policy (pass None, with max_agents and num_stack)")
        if not BP._is_int(max_agents) or max_agents not in (64, 128):
            raise ValueError(WHO + "max_agents must be 64 or 128, got %r" % (max_agents,))
        if not BP._is_int(num_stack) or not 1 <= num_stack <= 8:
            raise ValueError(WHO + "num_stack must be an int in [1, 8], got %r" % (num_stack,))
        A, R = max_agents, num_stack
    else:
        if not isinstance(policy, BP.DeviceBCPolicy):
            raise ValueError(WHO + "policy must be a DeviceBCPolicy for model %r" % (model,))
        if policy.network_dim != 64:
            raise ValueError(WHO + "the probes read 64-wide tokens: the policy's network_dim must be 64, got %d" % policy.network_dim)
        if max_agents not in (None, policy.max_agents) or num_stack not in (None, policy.num_stack):
            raise ValueError(WHO + "max_agents and num_stack are the policy's (%d, %d)" % (policy.max_agents, policy.num_stack))
        A, R = policy.max_agents, policy.num_stack
    K = in_features(model, exp, R)
    if K > 64:
        raise ValueError(WHO + "the baseline probe of exp 'other' has 12 * num_stack = %d input features; at most 64 are built" % K)
    try:
        b1, b2 = betas
    except (TypeError, ValueError):
        raise ValueError(WHO + "betas must be a pair of numbers")
    if not (_number(b1) and _number(b2) and 0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
        raise ValueError(WHO + "betas must lie in [0, 1), got %r" % (betas,))
    for name, v in (("lr", lr), ("eps", eps)):
        if not _number(v) or not v > 0:
            raise ValueError(WHO + "%s must be a positive number, got %r" % (name, v))
    if not _number(weight_decay) or weight_decay < 0:
        raise ValueError(WHO + "weight_decay must be a finite number that is not negative, got %r" % (weight_decay,))
    if partials is None:
        partials = DEFAULT_PARTIALS
    if not BP._is_int(partials) or not 1 <= partials <= MAX_PARTIALS:
        raise ValueError(WHO + "partials must be an int in [1, %d], got %r" % (MAX_PARTIALS, partials))
    check_state_dict(state_dict, K)
    return A, R, K, partials


def check_state_dict(sd, K, device=None):
    if not hasattr(sd, "keys") or not hasattr(sd, "__getitem__"):
        raise ValueError(WHO + "state_dict must be a mapping of names to tensors")
    keys = set(sd.keys())
    missing, extra = sorted(set(KEYS) - keys), sorted(keys - set(KEYS))
    if missing:
        raise ValueError(WHO + "missing key(s) %s" % ", ".join(map(repr, missing)))
    if extra:
        raise ValueError(WHO + "unexpected key(s) %s" % ", ".join(map(repr, extra)))
    for name, shape in zip(KEYS, ((CLASSES, K), (CLASSES,))):
        t = sd[name]
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape:
            raise ValueError(WHO + "%s must be a tensor of shape %s, got %s"
                             % (name, shape, tuple(t.shape) if isinstance(t, torch.Tensor) else type(t)))
        if t.dtype != torch.float32:
            raise ValueError(WHO + "%s must be float32, got %s" % (name, t.dtype))
        if not t.is_contiguous():
            raise ValueError(WHO + "%s must be contiguous" % name)
        if device is not None and t.device.type == "cuda" and t.device != device:
            raise ValueError(WHO + "%s is on %s, the probe on %s" % (name, t.device, device))


class DeviceLinearProbe:
    def __init__(self, policy, state_dict, model="early_lp", exp="other", lr=0.0015, eps=1e-4, *, betas=(0.9, 0.999),
                 weight_decay=0.01, chunk_rows=None, partials=None, max_agents=None, num_stack=None, device="cuda"):
        """policy: the `DeviceBCPolicy` to probe (None with model='baseline', which needs max_agents and num_stack instead).
        state_dict: 'head.weight' [64, K] and 'head.bias' [64], float32 (`nn.Linear(K, 64).state_dict()` under 'head.').
        lr, eps: lp.yaml's and linear_probing.py:148's; betas and weight_decay torch's AdamW defaults.  chunk_rows: the samples
        per chunk (None: the policy's; another value gives the probe a token scratch of its own).  partials: the partial sums
        of the gradient (None: 128).  Everything is allocated here, once.  Anything refused is a ValueError raised before
        anything reaches the device."""
        A, R, K, self.partials = check_probe_args(policy, state_dict, model, exp, lr, eps, betas, weight_decay, partials,
                                                  max_agents, num_stack)
        if chunk_rows is not None and (not BP._is_int(chunk_rows) or not 1 <= chunk_rows <= BP.MAX_CHUNK):
            raise ValueError(WHO + "chunk_rows must be an int in [1, %d], got %r" % (BP.MAX_CHUNK, chunk_rows))
        if policy is not None:
            dev = policy.device
        else:
            try:
                dev = torch.device(device)
            except (RuntimeError, TypeError) as e:
                raise ValueError(WHO + "device: %s" % e)
            if dev.type != "cuda":
                raise ValueError(WHO + "the probe runs on the GPU (there is no host path), got device %r" % (device,))
            dev = dev if dev.index is not None else torch.device("cuda", torch.cuda.current_device())
        check_state_dict(state_dict, K, dev)
        self.policy, self.model, self.exp, self.device = policy, model, exp, dev
        self.max_agents, self.num_stack, self.in_features = A, R, K
        self.obs_width = BP.obs_width(A)
        self.lr, self.eps, self.betas, self.weight_decay = float(lr), float(eps), (float(betas[0]), float(betas[1])), float(weight_decay)
        self.chunk_rows = policy.chunk_rows if policy is not None and chunk_rows is None else chunk_rows
        self._L = _capi.lib()
        G = self.G = CLASSES * K + CLASSES
        f = torch.float32
        self._own = []

        def new(shape, dtype=f, fill=None):
            t = torch.empty(shape, dtype=dtype, device=dev) if fill is None else torch.full(shape, fill, dtype=dtype, device=dev)
            self._own.append(t)
            return t

        self._scratch = None
        if policy is not None and self.chunk_rows != policy.chunk_rows:
            self._scratch = new((BP.scratch_floats(A, self.chunk_rows),))
        self.flat = new((G + 1,), fill=0.0)  # head.weight, head.bias, and the zero the padding columns are packed from
        self.packed = new((4096 + CLASSES,))
        self._index = new((4096 + CLASSES,), torch.int64)
        self._index.copy_(torch.from_numpy(pack_index(K)))
        self.exp_avg, self.exp_avg_sq, self.grad = new((G,), fill=0.0), new((G,), fill=0.0), new((G,), fill=0.0)
        self._part_f = new((self.partials, G))
        self._part_d = new((self.partials, 2), torch.float64)
        self._part_i = new((self.partials, _capi.LP_PART_INTS), torch.int32)
        self.stats = new((len(_capi.LP_STATS),), fill=0.0)
        self._lr, self._step = new((1,), fill=self.lr), new((1,), torch.int32, fill=0)
        self._beta_pow = new((2,), torch.float64, fill=1.0)
        self._scal = new((4,), fill=0.0)
        # what losses() reads, in one buffer: three float64 running sums, then steps, skipped, bad_labels
        self._read = new((10,), torch.int32, fill=0)
        self._sums, self._counts = self._read[:6].view(torch.float64), self._read[6:9]
        self._acc = new((_capi.LP_EVAL_WORDS,), torch.int32, fill=0)
        self._best = new((G,), fill=0.0)
        self._has_best = False
        self.best_loss = BEST_LOSS_START
        self.host_reads = 0
        self._load(state_dict)
        lp = self._lp = _capi.GdLPProbe()
        lp.model, lp.exp, lp.in_features, lp.num_partials = MODELS[model], EXPS[exp], K, self.partials
        lp.max_agents, lp.num_stack, lp.eps, lp.weight_decay = A, R, self.eps, self.weight_decay
        lp.beta1, lp.beta2 = self.betas
        lp.weight, lp.packed, lp.exp_avg, lp.exp_avg_sq = (t.data_ptr() for t in (self.flat, self.packed, self.exp_avg, self.exp_avg_sq))
        lp.lr, lp.step, lp.beta_pow, lp.grad = (t.data_ptr() for t in (self._lr, self._step, self._beta_pow, self.grad))
        lp.part_f, lp.part_d, lp.part_i = self._part_f.data_ptr(), self._part_d.data_ptr(), self._part_i.data_ptr()
        lp.stats, lp.sums, lp.counts, lp.scal = self.stats.data_ptr(), self._sums.data_ptr(), self._counts.data_ptr(), self._scal.data_ptr()

    @property
    def nbytes(self):
        """Everything the probe allocates beyond the policy: the weights in both layouts and the pack index, both moments, the
        gradient and its partials, the counters' partials, the best copy, the scalars (and a token scratch only when
        chunk_rows differs from the policy's)."""
        return sum(t.numel() * t.element_size() for t in self._own)

    @property
    def rows_per_sample(self):
        return self.max_agents - 1 if self.exp == "other" else 1

    # ---- weights

    def _load(self, sd):
        with torch.no_grad():
            self.flat[:self.G].copy_(torch.cat([sd[k].detach().to(self.device).reshape(-1) for k in KEYS]))
            torch.index_select(self.flat, 0, self._index, out=self.packed)

    def load_state_dict(self, state_dict):
        """New head weights (the same keys, shapes and dtype; ValueError otherwise), packed on the device.  The optimiser state
        stays."""
        check_state_dict(state_dict, self.in_features, self.device)
        self._load(state_dict)

    def _views(self, flat):
        K = self.in_features
        return {"head.weight": flat[:CLASSES * K].view(CLASSES, K), "head.bias": flat[CLASSES * K:CLASSES * K + CLASSES]}

    def state_dict(self):
        """'head.weight' [64, K] and 'head.bias' [64]: clones of the flat buffer's views."""
        return {k: v.clone() for k, v in self._views(self.flat).items()}

    def best_state_dict(self):
        """The weights of the evaluation with the smallest summed loss `fit` has seen (the reference's best checkpoint,
        linear_probing.py:327-332); None before the first."""
        return {k: v.clone() for k, v in self._views(self._best).items()} if self._has_best else None

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
        if not 1 <= B <= BP.MAX_ROWS:
            raise ValueError(WHO + "B must be in [1, %d], got %d" % (BP.MAX_ROWS, B))
        self._tensor("obs", obs, (torch.float32,), (B, R, self.obs_width))
        self._tensor("partner_mask", partner_mask, (torch.bool, torch.uint8), (B, R, A - 1))
        self._tensor("road_mask", road_mask, (torch.bool, torch.uint8), (B, R, BP.ROADS))
        return B

    def _row_shape(self, B):
        return (B, self.max_agents - 1) if self.exp == "other" else (B,)

    def _labels(self, mask, labels, B):
        names = ("aux_mask", "other_pos") if self.exp == "other" else ("future_valid_mask", "ego_pos")
        shape = self._row_shape(B)
        for name, t, dts in ((names[0], mask, (torch.bool, torch.uint8)), (names[1], labels, (torch.int64,))):
            if isinstance(t, torch.Tensor) and tuple(t.shape) != shape and t.dim() != len(shape):
                raise ValueError(WHO + "exp is %r: the batch's last two tensors must be %s and %s of shape %s, got a %s of shape %s "
                                 "(a dataset of the other exp?)" % (self.exp, names[0], names[1], shape, name, tuple(t.shape)))
            self._tensor(name, t, dts, shape)
        if labels.data_ptr() % 8:
            raise ValueError(WHO + "%s must be 8-byte aligned" % names[1])

    def _policy_struct(self):
        if self.policy is None:
            return None
        p = self.policy.c_struct()  # the blob as it is NOW: the probe follows a policy that is still training
        if self._scratch is not None:
            p.chunk_rows, p.scratch, p.scratch_floats = self.chunk_rows, self._scratch.data_ptr(), self._scratch.numel()
        return p

    def _call(self, fn, name, obs, pm, rm, B, *rest):
        p = self._policy_struct()
        with torch.cuda.device(self.device):
            stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            _capi.check(fn(None if p is None else C.byref(p), C.byref(self._lp), obs.data_ptr(), pm.data_ptr(), rm.data_ptr(), B,
                           *rest, stream), name)

    def _rows(self, B, logits=None, loss_row=None, pred=None):
        shape = self._row_shape(B)
        r = _capi.GdLPRows()
        if logits is not None:
            self._tensor("out logits", logits, (torch.float32,), shape + (CLASSES,))
            if logits.data_ptr() % 16:
                raise ValueError(WHO + "out logits must be 16-byte aligned")
            r.logits = logits.data_ptr()
        if loss_row is not None:
            r.loss_row = self._tensor("out loss_row", loss_row, (torch.float32,), shape).data_ptr()
        if pred is not None:
            self._tensor("out pred", pred, (torch.int64,), shape)
            if pred.data_ptr() % 8:
                raise ValueError(WHO + "out pred must be 8-byte aligned")
            r.pred = pred.data_ptr()
        return r

    # ---- the calls

    def logits(self, obs, partner_mask, road_mask, out=None):
        """LinearProbPosition.forward on the tapped tokens: [B, A - 1, 64] for 'other', [B, 64] for 'ego'.  One C call
        (`gd_lp_forward`); no host synchronisation, with out= no allocation."""
        B = self._inputs(obs, partner_mask, road_mask)
        if out is None:
            out = torch.empty(self._row_shape(B) + (CLASSES,), dtype=torch.float32, device=self.device)
        rows = self._rows(B, logits=out)
        self._call(self._L.gd_lp_forward, "gd_lp_forward", obs, partner_mask, road_mask, B, C.byref(rows))
        return out

    def predict(self, obs, partner_mask, road_mask, out=None):
        """LinearProbPosition.predict: the first class of the largest logit, int64 [B, A - 1] or [B]."""
        B = self._inputs(obs, partner_mask, road_mask)
        if out is None:
            out = torch.empty(self._row_shape(B), dtype=torch.int64, device=self.device)
        rows = self._rows(B, pred=out)
        self._call(self._L.gd_lp_forward, "gd_lp_forward", obs, partner_mask, road_mask, B, C.byref(rows))
        return out

    def update(self, obs, actions, valid_mask, ego_mask, partner_mask, road_mask, mask, labels, *, logits=None, loss_row=None,
               pred=None):
        """One gradient step on the eight tensors `DeviceFutureDataset.batch` writes, as they are (actions, valid_mask and
        ego_mask are not read, as in the reference).  mask / labels: aux_mask / other_pos [B, A - 1] for exp 'other',
        future_valid_mask / ego_pos [B] for 'ego'.  ONE C call (`gd_lp_update`) on torch's current stream, no host
        synchronisation, no allocation.  logits, loss_row, pred: tensors to receive the per-row values.  Afterwards the weights
        in both layouts, the moments, `grad` and `stats` are the step's -- unless the batch selected no row, which only
        advances `skipped`."""
        B = self._inputs(obs, partner_mask, road_mask)
        self._labels(mask, labels, B)
        rows = self._rows(B, logits, loss_row, pred)
        self._call(self._L.gd_lp_update, "gd_lp_update", obs, partner_mask, road_mask, B, mask.data_ptr(), labels.data_ptr(),
                   C.byref(rows))

    def _counts_now(self):
        self.host_reads += 1
        return [int(v) for v in self._counts.cpu().tolist()]

    def fit(self, ds, total_gradient_steps, batch_size=256, eval_ds=None, eval_freq=None, generator=None):
        """The reference's loop (linear_probing.py:158-341): shuffled epochs of `ds.batches(batch_size)`, an `update` per
        batch, until total_gradient_steps steps are made, in mid-epoch if that is where the count is reached.  A batch that
        selects no row is no step.  The device decides that, so the host counts every batch as a step until the count reaches
        the next evaluation or the end and only THEN reads the device's own count (one read); where batches were skipped it
        goes on.  Every eval_freq steps `evaluate(eval_ds, batch_size)` runs, and whenever its summed loss improves a device
        copy of the weights is kept (`best_state_dict`).  Returns the evaluations made, as a list of (step, dict)."""
        self._check_dataset(ds, "fit")
        if not BP._is_int(total_gradient_steps) or total_gradient_steps < 0:
            raise ValueError(WHO + "fit: total_gradient_steps must be an int that is not negative, got %r" % (total_gradient_steps,))
        if not BP._is_int(batch_size) or not 1 <= batch_size <= BP.MAX_ROWS:
            raise ValueError(WHO + "fit: batch_size must be an int in [1, %d], got %r" % (BP.MAX_ROWS, batch_size))
        if (eval_ds is None) != (eval_freq is None):
            raise ValueError(WHO + "fit: eval_ds and eval_freq go together")
        if eval_ds is not None:
            self._check_dataset(eval_ds, "fit: eval_ds")
            if not BP._is_int(eval_freq) or eval_freq < 1:
                raise ValueError(WHO + "fit: eval_freq must be a positive int, got %r" % (eval_freq,))
        if len(ds) == 0:
            raise ValueError(WHO + "fit: the dataset is empty")
        evals = []
        if total_gradient_steps == 0:
            return evals
        base = self._counts_now()[0]
        steps, pending = 0, 0  # the steps the device has confirmed; the batches issued since

        def milestone():
            return total_gradient_steps if eval_freq is None else min(total_gradient_steps, (steps // eval_freq + 1) * eval_freq)

        target = milestone()
        while True:
            before = steps
            for batch in ds.batches(batch_size, shuffle=True, generator=generator):
                self.update(*batch)
                pending += 1
                if steps + pending < target:
                    continue
                steps, pending = self._counts_now()[0] - base, 0  # never above target: it is read as soon as it could be there
                if steps < target:
                    continue
                if eval_freq is not None and steps % eval_freq == 0:
                    raw = self._evaluate(eval_ds, batch_size)
                    if raw["loss_sum"] < self.best_loss:
                        self.best_loss = raw["loss_sum"]
                        self._best.copy_(self.flat[:self.G])
                        self._has_best = True
                    evals.append((steps, raw["public"]))
                if steps >= total_gradient_steps:
                    return evals
                target = milestone()
            if pending:
                steps, pending = self._counts_now()[0] - base, 0
            if steps == before:
                raise ValueError(WHO + "fit: a whole epoch selected no row")

    def losses(self):
        """The means over the updates since the last call that were not skipped of pos_loss, pos_accuracy and pos_f1_macro
        (linear_probing.py:335-341), and steps, skipped and bad_labels over the same span: ONE read of the device (counted in
        `host_reads`), after which the sums start again.  With no step since the last call the means are 0."""
        host = self._read.cpu()
        self.host_reads += 1
        self._read.zero_()
        sums = host[:6].view(torch.float64).tolist()
        steps, skipped, bad = (int(v) for v in host[6:9].tolist())
        out = {k: (s / steps if steps else 0.0) for k, s in zip(TRAIN_NAMES, sums)}
        out.update(steps=steps, skipped=skipped, bad_labels=bad)
        return out

    def _check_dataset(self, ds, what):
        if hasattr(ds, "batches") and hasattr(ds, "__len__"):
            if getattr(ds, "exp", self.exp) != self.exp:
                raise ValueError(WHO + "%s: the dataset's exp is %r, the probe's %r" % (what, ds.exp, self.exp))
            if getattr(ds, "rollout_len", self.num_stack) != self.num_stack or getattr(ds, "max_agents", self.max_agents) != self.max_agents:
                raise ValueError(WHO + "%s: the dataset has rollout_len %r and %r agents, the probe num_stack %d and %d agents"
                                 % (what, getattr(ds, "rollout_len", None), getattr(ds, "max_agents", None), self.num_stack,
                                    self.max_agents))
        elif not hasattr(ds, "__iter__"):
            raise ValueError(WHO + "%s: a DeviceFutureDataset or an iterable of its batches is expected" % what)

    def _evaluate(self, ds, batch_size):
        self._check_dataset(ds, "evaluate")
        if hasattr(ds, "batches"):
            if not BP._is_int(batch_size) or batch_size < 1:
                raise ValueError(WHO + "evaluate: batch_size must be a positive int, got %r" % (batch_size,))
            batches = ds.batches(batch_size, shuffle=False)
        else:
            batches = ds
        self._acc.zero_()
        rows = _capi.GdLPRows()
        for batch in batches:
            obs, _, _, _, pm, rm, mask, labels = batch
            B = self._inputs(obs, pm, rm)
            self._labels(mask, labels, B)
            self._call(self._L.gd_lp_eval_accumulate, "gd_lp_eval_accumulate", obs, pm, rm, B, mask.data_ptr(), labels.data_ptr(),
                       C.byref(rows), self._acc.data_ptr())
        host = self._acc.cpu()  # the one host read
        self.host_reads += 1
        d = host[:8].view(torch.float64).tolist()
        i = host[8:].numpy().astype(np.int64)
        n, skipped, ood_correct, ood_rows, bad = (int(v) for v in i[:5])
        cnt = i[8:8 + 3 * CLASSES].reshape(3, CLASSES)
        nan = float("nan")
        pub = {"eval/pos_accuracy": d[1] / n if n else nan, "eval/pos_loss": d[0] / n if n else nan,
               "eval/pos_f1_macro": d[2] / n if n else nan,
               "eval/ood_accuracy": ood_correct / ood_rows if ood_rows else nan, "eval/ood_loss": d[3] / ood_rows if ood_rows else nan,
               "eval/ood_f1_macro": macro_f1(cnt[0], cnt[1], cnt[2]),
               "batches": n, "skipped": skipped, "ood_rows": ood_rows, "bad_labels": bad}
        return dict(public=pub, loss_sum=d[0])

    def evaluate(self, ds, batch_size=256):
        """The reference's evaluation (linear_probing.py:235-326) on the current weights.  ds: a `DeviceFutureDataset` (its
        batches of batch_size in index order) or an iterable of its batches.  Per batch one C call (`gd_lp_eval_accumulate`);
        the sums stay on the device and are read ONCE at the end.  The averaging is the reference's: eval/pos_accuracy,
        eval/pos_loss and eval/pos_f1_macro are per-batch means averaged over the batches that selected a row;
        eval/ood_accuracy and eval/ood_loss are global sums over the global OOD row count (nan at 0 / 0); eval/ood_f1_macro
        comes from the per-class counters summed over all batches.  Also: batches, skipped, ood_rows, bad_labels."""
        return self._evaluate(ds, batch_size)["public"]

    # ---- the optimiser's state

    def set_learning_rate(self, x):
        if not _number(x) or not x > 0:
            raise ValueError(WHO + "set_learning_rate: a positive number, got %r" % (x,))
        self.lr = float(x)
        self._lr.fill_(self.lr)

    def optimizer_state_dict(self):
        """`torch.optim.AdamW.state_dict()`'s format over (head.weight, head.bias): `step` (a float32 scalar, as torch keeps it),
        `exp_avg`, `exp_avg_sq`; one param group with this torch's own keys.  It loads into a `torch.optim.AdamW` over an
        `nn.Linear(K, 64)`'s parameters, and that optimiser's loads here.  (One host read: the step count.)"""
        step = float(self._step.item())
        self.host_reads += 1
        m, v = self._views(self.exp_avg), self._views(self.exp_avg_sq)
        state = {i: {"step": torch.tensor(step), "exp_avg": m[k].clone(), "exp_avg_sq": v[k].clone()} for i, k in enumerate(KEYS)}
        probe = torch.optim.AdamW([torch.zeros(1)], lr=self.lr, betas=self.betas, eps=self.eps, weight_decay=self.weight_decay,
                                  amsgrad=False)
        group = dict(probe.state_dict()["param_groups"][0])
        group["params"] = [0, 1]
        return {"state": state, "param_groups": [group]}

    def load_optimizer_state_dict(self, sd):
        """The inverse: moments and step count from a `torch.optim.AdamW` state dict over the same two parameters (an empty
        state is a fresh optimiser), and the learning rate and weight decay of its param group.  Its betas and eps must be
        this object's.  The running products of the betas are rebuilt by `step` float64 multiplications, as the kernel builds
        them."""
        who = WHO + "load_optimizer_state_dict: "
        try:
            state, groups = sd["state"], sd["param_groups"]
        except (TypeError, KeyError):
            raise ValueError(who + "not an optimiser state dict")
        if len(groups) != 1 or list(groups[0].get("params", ())) != [0, 1]:
            raise ValueError(who + "one param group over the 2 parameters is expected")
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
        if len(state) not in (0, 2) or (state and sorted(state) != [0, 1]):
            raise ValueError(who + "state for none or both of the 2 parameters is expected")
        try:
            steps = {int(float(state[i]["step"])) for i in state} or {0}
        except (TypeError, KeyError, ValueError):
            raise ValueError(who + "every parameter's state must carry step, exp_avg and exp_avg_sq")
        if len(steps) != 1 or min(steps) < 0:
            raise ValueError(who + "every parameter must carry the same non-negative step")
        shapes = ((CLASSES, self.in_features), (CLASSES,))
        for i, shape in enumerate(shapes):
            if state and any(not isinstance(state[i].get(k), torch.Tensor) or tuple(state[i][k].shape) != shape
                             or state[i][k].dtype != torch.float32 for k in ("exp_avg", "exp_avg_sq")):
                raise ValueError(who + "parameter %d: float32 moments of shape %s are expected" % (i, shape))
        step = steps.pop()
        for name, mine in (("exp_avg", self.exp_avg), ("exp_avg_sq", self.exp_avg_sq)):
            for i, k in enumerate(KEYS):
                view = self._views(mine)[k]
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
        self.weight_decay = self._lp.weight_decay = float(wd)
        if "lr" in group:
            self.set_learning_rate(group["lr"])
