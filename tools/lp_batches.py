#!/usr/bin/env python3
"""Linear-probing batches from one recorded expert episode: tools/il_batches.py's workload (ppo_default, --worlds x 128 slots,
rollout_len 5, pred_len 1, batch size 512), its selection pool and its alternation in one process, at future_step 35, one JSON
line:

  (a) DeviceFutureDataset.batch(sel) for exp='other' and exp='ego': one kernel launch (gd_il_future_batch);
  (b) DeviceExpertDataset.batch(sel) plus valid_mask, ego_mask, the future mask and the labels composed in torch on the device
      (gathers of the poses, of the partner block of the future observation row and of two partner mask rows; fp32 eager
      arithmetic in the rule's order, cos / sin in double; torch.bucketize against the double edges), checked equal to (a)
      before anything is timed;
  (c) DeviceExpertDataset.batch(sel) alone: the yardstick, the same measurement as (a) of tools/il_batches.py.

Reported: the median and the range of the microseconds per batch of each, (a) as a ratio to (c), and the bytes exp='other'
moves per sample beyond the window.
tools/lp_batches.py [--worlds 1024] [--runs 3] [--batches 1000] [--out FILE]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

import bench  # noqa: E402
from il_batches import B, POOL, P, R, T, WORKLOAD, record, summary, timed  # noqa: E402

F = 35


class TorchComposition:
    """(b): the plain dataset's batch and the other four outputs from torch operations.  rows / idx2: the index, per sample;
    valid: gd_il_index's flag per (row, time), computed once."""

    def __init__(self, ep, plain, fut):
        N, _, D = ep.obs.shape
        self.plain, self.exp, self.PM = plain, fut.exp, plain.max_agents - 1
        e = plain._entries[:len(plain)].to(torch.int64)
        self.rows, self.idx2 = e[:, 1].contiguous(), e[:, 2].contiguous()
        a = ep.actions.abs()
        self.valid = (~ep.dead_mask & ~((a[..., 1] > 0.5) | (a[..., 0] > 5) | (a[..., 2] > 0.2))).view(N * T)
        self.block = ep.obs.view(N * T, D)[:, 6:6 + 6 * self.PM]  # (a view: indexing it gathers these columns only)
        self.partner = ep.partner_mask.view(N * T, self.PM)
        self.pos, self.rot = ep.ego_global_pos.view(N * T, 2), ep.ego_global_rot.view(N * T)
        dev = ep.obs.device
        self.window = torch.arange(R, device=dev) - (R - 1)
        self.xb, self.yb = (torch.tensor(b, dtype=torch.float64, device=dev) for b in (fut.xbins, fut.ybins))

    def label(self, x, y):
        def cls(v, b):
            k = torch.bucketize(v.double(), b, right=True) - 1
            return torch.where(v.isnan(), 7, k.clamp_(0, 7))
        return cls(x, self.xb) * 8 + cls(y, self.yb)

    @staticmethod
    def norm(v):
        return 2 * ((v - (-1000)) / 2000) - 1

    @staticmethod
    def cos_sin(a):
        a = a.double()
        return a.cos().float(), a.sin().float()

    def batch(self, sel):
        obs, actions, partner_mask, road_mask, _ = self.plain.batch(sel)
        rows, idx2 = self.rows[sel], self.idx2[sel]
        now = rows * T + idx2
        ahead = idx2 + F < T
        fut = rows * T + (idx2 + F).clamp_(max=T - 1)
        valid_mask = self.valid[now + (P - 1)]
        times = idx2[:, None] + self.window
        ego_mask = self.valid[rows[:, None] * T + times.clamp(min=0)] & (times >= 0)
        here, there = self.pos[now], self.pos[fut]
        if self.exp == "ego":
            mask = self.valid[now] & ahead & self.valid[fut]
            d = there - here
            c, s = self.cos_sin(self.rot[now])
            rx, ry = d[:, 0] * c + d[:, 1] * s, (-d[:, 0]) * s + d[:, 1] * c
            zero = ~ahead
        else:
            mask = (self.partner[now] != 0) | ~ahead[:, None] | (self.partner[fut] != 0)
            blk = self.block[fut].view(-1, self.PM, 6)
            px, py = blk[..., 1] * 1000, blk[..., 2] * 1000
            c, s = (v[:, None] for v in self.cos_sin(self.rot[fut]))
            gx, gy = (there[:, 0, None] + px * c) - py * s, (there[:, 1, None] + px * s) + py * c
            dx, dy = gx - here[:, 0, None], gy - here[:, 1, None]
            c2, s2 = (v[:, None] for v in self.cos_sin(-self.rot[now]))
            rx, ry = dx * c2 + dy * s2, (-dx) * s2 + dy * c2
            zero = mask
        x, y = self.norm(rx).masked_fill_(zero, 0.0), self.norm(ry).masked_fill_(zero, 0.0)
        return obs, actions, valid_mask, ego_mask, partner_mask, road_mask, mask, self.label(x, y)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worlds", type=int, default=1024)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--batches", type=int, default=1000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    os.environ.pop("GPUDRIVE_IL_SPLIT", None)
    res = dict(tool="tools/lp_batches.py", workload=WORKLOAD, worlds=args.worlds, runs=args.runs, batches=args.batches,
               rollout_len=R, pred_len=P, batch_size=B, future_step=F, source_stamp=bench.source_stamp())
    ep, A = record(args.worlds)
    plain = ep.dataset(rollout_len=R, pred_len=P)
    futs = {exp: ep.future_dataset(rollout_len=R, pred_len=P, future_step=F, exp=exp) for exp in ("other", "ego")}
    comps = {exp: TorchComposition(ep, plain, ds) for exp, ds in futs.items()}
    M = len(plain)
    res.update(slots=A, rows=int(ep.obs.shape[0]), samples=M, index_bytes=plain.nbytes)
    assert all(len(ds) == M and torch.equal(ds.valid_indices, plain.valid_indices) for ds in futs.values())
    g = torch.Generator(device="cuda").manual_seed(0)
    pool = list(plain.batch_selections(torch.randperm(M, device="cuda", generator=g)[:POOL * B].contiguous(), B))
    assert len(pool) == POOL and all(s.numel() == B for s in pool), "the recording is too small for the pool"

    # (a) against (b) before timing: eight selections of the pool, the samples whose window crosses t = 0 and the ones whose
    # future lies past the episode's end
    vi = plain.valid_indices
    first = torch.cat(pool[:8] + [(vi[:, 1] < R - 1).nonzero().squeeze(1)[:448], (vi[:, 1] + F >= T).nonzero().squeeze(1)[:448]])
    bits = lambda x: x.contiguous().view(torch.int32) if x.dtype == torch.float32 else x
    names = ("obs", "actions", "valid_mask", "ego_mask", "partner_mask", "road_mask", "future_mask", "future_pos")
    for exp in futs:
        a, b = futs[exp].batch(first), comps[exp].batch(first)
        same = {n: bool(torch.equal(bits(x), bits(y))) for n, x, y in zip(names, a, b)}
        unmasked = ~a[6] if exp == "other" else torch.ones_like(a[6])
        res["check_" + exp] = dict(samples=int(first.numel()), equal=same, labels=int(a[7].numel()),
                                   labels_unmasked=int(unmasked.sum()), labels_differing=int((a[7] != b[7]).sum()),
                                   classes_seen=int(a[7][unmasked].unique().numel()))
    res["a_equals_b"] = all(all(res["check_" + exp]["equal"].values()) for exp in futs)

    variants = dict(a_other=futs["other"].batch, a_ego=futs["ego"].batch, b_other=comps["other"].batch, b_ego=comps["ego"].batch,
                    c=plain.batch)
    us = {k: [] for k in variants}
    for _ in range(args.runs):
        for k, fn in variants.items():
            us[k].append(timed(fn, pool, args.batches))
    res.update({k: summary(v) for k, v in us.items()})
    c = res["c"]["median"]
    res.update(a_other_over_c=res["a_other"]["median"] / c, a_ego_over_c=res["a_ego"]["median"] / c,
               b_other_over_a_other=res["b_other"]["median"] / res["a_other"]["median"],
               b_ego_over_a_ego=res["b_ego"]["median"] / res["a_ego"]["median"],
               c_range_over_median=(res["c"]["hi"] - res["c"]["lo"]) / c)
    # what exp='other' moves per sample beyond the plain batch: the partner block of one observation row and two partner mask
    # rows read, the labels and aux_mask written, valid_mask and ego_mask written, data_idx not written
    PM = A - 1
    res["other_extra_bytes_per_sample"] = (6 + 6 * PM) * 4 + 2 * PM + PM * 8 + PM + 1 + R - 16
    res["window_bytes_per_sample"] = R * (ep.obs.shape[2] * 4 + PM + 200)
    res["bad_indices"] = [int(ds.bad_indices) for ds in (plain, futs["other"], futs["ego"])]
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    with torch.cuda.stream(torch.cuda.Stream()):  # (the step graph is captured on a stream of torch's own, as in bench.py)
        main()
