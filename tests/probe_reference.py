"""The linear probe restated in float64 numpy, in this repository's own words: what gd_bc_hidden, gd_lp_forward, gd_lp_update
and gd_lp_eval_accumulate are held to.  The taps are composed from bc_reference's public unpack, embed and self_layer;
tests/test_lp_probe.py pins taps, logits and loss to the reference's own modules (tests/golden/lp_probe_*.npz)."""
import numpy as np

from . import bc_reference as REF

CLASSES = 64


def taps(sd, obs, partner_mask, road_mask, max_agents, num_layer):
    """{'fusion_attn', 'ro_attn'}: tokens 0 .. A - 1 of the block's last_hidden_state, [B, A, 64] float64; and under the key
    (tap, i) the same tokens after layer i of that block (what `hidden(tap=, layer=i)` taps)."""
    sd = REF._sd64(sd)
    obs = np.asarray(obs, dtype=np.float64)
    A, B = max_agents, obs.shape[0]
    pm = np.asarray(partner_mask).astype(bool)[:, -1]
    rm = np.asarray(road_mask).astype(bool)[:, -1]
    ego, ro, rg = REF.unpack(obs, A)
    x = np.concatenate([REF.embed(ego, sd, "ego_state_net")[:, None], REF.embed(ro, sd, "road_object_net"),
                        REF.embed(rg, sd, "road_graph_net")], axis=1)
    ego_mask = np.zeros((B, 1), dtype=bool)
    all_mask, obj_mask = np.concatenate([ego_mask, pm, rm], 1), np.concatenate([ego_mask, pm], 1)
    out = {}
    for i in range(num_layer[0]):
        x = REF.self_layer(x, all_mask, sd, "fusion_attn.%d" % i)
        out[("fusion_attn", i)] = x[:, :A].copy()
    out["fusion_attn"] = x[:, :A].copy()
    objs = x[:, :A]
    for i in range(num_layer[1]):
        objs = REF.self_layer(objs, obj_mask, sd, "ro_attn.%d" % i)
        out[("ro_attn", i)] = objs.copy()
    out["ro_attn"] = objs
    return out


def rows(hidden, exp):
    """The probe's input rows from a tap [B, A, 64]: token 0 for 'ego' [B, 64], tokens 1 .. A - 1 for 'other' [B, A - 1, 64]."""
    return hidden[:, 0] if exp == "ego" else hidden[:, 1:]


def baseline_rows(obs, max_agents, exp):
    """The baseline probe's rows (linear_probing.py:183-191): 'ego' obs[b, :, :6] flattened [B, 6 R]; 'other' per partner j
    [ego 6 | partner j's 6] per time index, in time order [B, A - 1, 12 R]."""
    obs = np.asarray(obs, dtype=np.float64)
    B, R, _ = obs.shape
    A = max_agents
    ego = obs[:, :, :6]
    if exp == "ego":
        return ego.reshape(B, R * 6)
    partners = obs[:, :, 6:6 * A].reshape(B, R, A - 1, 6)
    both = np.concatenate([np.broadcast_to(ego[:, :, None, :], (B, R, A - 1, 6)), partners], axis=-1)
    return both.transpose(0, 2, 1, 3).reshape(B, A - 1, R * 12)


def logits(x, head):
    w = np.asarray(head["head.weight"].detach().cpu().numpy() if hasattr(head["head.weight"], "detach") else head["head.weight"], np.float64)
    b = np.asarray(head["head.bias"].detach().cpu().numpy() if hasattr(head["head.bias"], "detach") else head["head.bias"], np.float64)
    return x @ w.T + b


def ood_set(exp):
    if exp == "other":
        return np.array([x * 8 + y for x in range(8) for y in range(8) if x in (0, 1, 6, 7) or y in (0, 1, 6, 7)])
    return np.array([x * 8 + y for x in range(8) for y in range(8) if x not in (3, 4)])


def macro_f1(pred, label):
    """sklearn's f1_score(average='macro') over the classes present in either array; nan for no rows."""
    pred, label = np.asarray(pred), np.asarray(label)
    if pred.size == 0:
        return float("nan")
    f = []
    for c in np.union1d(pred, label):
        tp = np.sum((pred == c) & (label == c))
        f.append(2.0 * tp / (np.sum(pred == c) + np.sum(label == c)))
    return float(np.mean(f))


def batch(z, x, mask, label, exp):
    """One batch from float64 logits z [.., 64] and rows x [.., K]: the selection (rows with a label outside [0, 63] dropped and
    counted), M, loss, accuracy, macro F1, the gradient of the mean loss [64 K + 64], the per-row values and the OOD figures."""
    z, x = z.reshape(-1, CLASSES), x.reshape(z.reshape(-1, CLASSES).shape[0], -1)
    label = np.asarray(label).reshape(-1)
    sel = (~np.asarray(mask).astype(bool) if exp == "other" else np.asarray(mask).astype(bool)).reshape(-1)
    ok = (label >= 0) & (label < CLASSES)
    use = sel & ok
    m = z.max(-1, keepdims=True)
    lse = m[:, 0] + np.log(np.exp(z - m).sum(-1))
    pred = z.argmax(-1)
    lab = np.where(ok, label, 0)
    loss_row = np.where(ok, lse - z[np.arange(len(z)), lab], 0.0)
    out = dict(use=use, M=int(use.sum()), bad=int((sel & ~ok).sum()), pred=pred, loss_row=loss_row)
    if out["M"] == 0:
        out.update(loss=float("nan"), accuracy=float("nan"), f1=float("nan"), grad=None, ood_rows=0, ood_loss_sum=0.0,
                   ood_correct=0, ood_pred=pred[:0], ood_label=lab[:0])
        return out
    g = np.exp(z - lse[:, None])
    g[np.arange(len(z)), lab] -= 1.0
    g = g * use[:, None] / out["M"]
    od = use & np.isin(lab, ood_set(exp))
    out.update(loss=float(loss_row[use].mean()), accuracy=float((pred == lab)[use].mean()), f1=macro_f1(pred[use], lab[use]),
               grad=np.concatenate([(g.T @ x).reshape(-1), g.sum(0)]), ood_rows=int(od.sum()), ood_loss_sum=float(loss_row[od].sum()),
               ood_correct=int((pred == lab)[od].sum()), ood_pred=pred[od], ood_label=lab[od])
    return out


def evaluate(batches):
    """The reference's evaluation (linear_probing.py:235-326) from per-batch `batch` results: per-batch means averaged over the
    batches that selected a row; OOD figures as global sums over the global count; the OOD F1 over all batches' rows."""
    live = [b for b in batches if b["M"] > 0]
    n, rows_ = len(live), sum(b["ood_rows"] for b in live)
    nan = float("nan")
    return {"eval/pos_accuracy": sum(b["accuracy"] for b in live) / n if n else nan,
            "eval/pos_loss": sum(b["loss"] for b in live) / n if n else nan,
            "eval/pos_f1_macro": sum(b["f1"] for b in live) / n if n else nan,
            "eval/ood_accuracy": sum(b["ood_correct"] for b in live) / rows_ if rows_ else nan,
            "eval/ood_loss": sum(b["ood_loss_sum"] for b in live) / rows_ if rows_ else nan,
            "eval/ood_f1_macro": macro_f1(np.concatenate([b["ood_pred"] for b in live]) if live else [],
                                          np.concatenate([b["ood_label"] for b in live]) if live else []),
            "batches": n, "skipped": len(batches) - n}
