#!/usr/bin/env python3
"""Imitation-learning batches from one recorded expert episode at ppo_default (Waymo tiles, --worlds x 128 slots, linear road
selection), with baselines/il/config/il.yaml's rollout_len 5, pred_len 1 and batch size 512, two ways, one JSON line:

  (a) DeviceExpertDataset.batch(sel): one kernel launch (gd_il_batch);
  (b) the best composition in torch alone on the device that makes no padded copy of the dataset: advanced indexing with
      clamped times, then the zero / True prefix by an in-place masked fill or an `|`, for all five outputs (its index is
      handed to it: only the gather is timed).

(a) and (b) alternate in one process, --runs each: device events around --batches batches after a warm-up, every batch with
another selection out of a pool drawn once (the pool's samples together are several times the 256 MB Infinity Cache, so a
repeat of a selection still reads HBM).  Reported: the median and the range of the microseconds per batch, whether (a)
equals (b) bit for bit, the index build time (a host clock around work that ends in a synchronise), and (a)'s algorithmic
bytes per batch (every output written once, and read once from the dataset what is not padding) over its time as a fraction
of the 6.29 TB/s copy ceiling.  Then the sweep behind GD_IL_SPLIT of il_batch.hip, the workgroups per sample, through the
developer switch GPUDRIVE_IL_SPLIT, the variants interleaved run by run.
bench.py's workload builders are imported, not changed.
tools/il_batches.py [--worlds 1024] [--runs 3] [--batches 1000] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402
from gpudrive_lab_amd.recorder import ExpertRecorder  # noqa: E402

WORKLOAD = "ppo_default"
T = 91
R, P, B = 5, 1, 512  # baselines/il/config/il.yaml
COPY_CEILING = 6.29e12
POOL = 64


def record(worlds):
    kw = bench.params_for(WORKLOAD)
    _, order, agents = bench.split_workload(WORKLOAD)
    scenes = bench.scenes_for(WORKLOAD, worlds, 0, agents=agents)
    sim = bench.make_sim(scenes, kw, agents, 0, knn_order=order)
    ep = ExpertRecorder(sim).record()
    torch.cuda.synchronize()
    sim.close()
    return ep, agents


class TorchComposition:
    """(b).  rows / idx2 / idx1: the index, per sample."""

    def __init__(self, ep, ds):
        N, _, D = ep.obs.shape
        A = ds.max_agents
        e = ds._entries[:len(ds)].to(torch.int64)
        self.rows, self.idx2, self.idx1 = e[:, 1].contiguous(), e[:, 2].contiguous(), e[:, 3].contiguous()
        self.obs, self.actions = ep.obs.view(N * T, D), ep.actions.view(N * T, 3)
        self.partner, self.road = ep.partner_mask.view(N * T, A - 1), ep.road_mask.view(N * T, 200)
        self.window = torch.arange(R, device=ep.obs.device) - (R - 1)
        self.ahead = torch.arange(P, device=ep.obs.device)

    def batch(self, sel):
        rows, idx2 = self.rows[sel], self.idx2[sel]
        times = idx2[:, None] + self.window
        pad = (times < 0)[..., None]
        at = rows[:, None] * T + times.clamp_(min=0)
        obs = self.obs[at].masked_fill_(pad, 0.0)
        actions = self.actions[(rows * T + idx2)[:, None] + self.ahead]
        partner = (self.partner[at] == 2).logical_or_(pad)
        road = self.road[at].logical_or_(pad)
        return obs, actions, partner, road, torch.stack((self.idx1[sel], idx2), 1)


def timed(fn, pool, batches, warm=20):
    for i in range(warm):
        fn(pool[i % POOL])
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for i in range(batches):
        fn(pool[i % POOL])
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / batches  # microseconds per batch


def summary(us):
    return dict(us=us, median=statistics.median(us), lo=min(us), hi=max(us))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worlds", type=int, default=1024)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--batches", type=int, default=1000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    os.environ.pop("GPUDRIVE_IL_SPLIT", None)
    res = dict(tool="tools/il_batches.py", workload=WORKLOAD, worlds=args.worlds, runs=args.runs, batches=args.batches,
               rollout_len=R, pred_len=P, batch_size=B, source_stamp=bench.source_stamp())
    ep, A = record(args.worlds)
    N, _, D = ep.obs.shape
    dataset_bytes = sum(getattr(ep, k).numel() * getattr(ep, k).element_size() for k in ep.ARRAYS)
    build = []
    for _ in range(args.runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ds = ep.dataset(rollout_len=R, pred_len=P)
        torch.cuda.synchronize()
        build.append((time.perf_counter() - t0) * 1e3)
    M = len(ds)
    res.update(slots=A, rows=N, kept_rows=int(ep.keep.sum()), samples=M, dataset_bytes=dataset_bytes, index_bytes=ds.nbytes,
               index_build_ms=build, index_build_ms_median=statistics.median(build))
    comp = TorchComposition(ep, ds)
    g = torch.Generator(device="cuda").manual_seed(0)
    pool = list(ds.batch_selections(torch.randperm(M, device="cuda", generator=g)[:POOL * B].contiguous(), B))
    assert len(pool) == POOL and all(s.numel() == B for s in pool), "the recording is too small for the pool"
    first = torch.cat([s[:8] for s in pool[:8]] + [(ds.valid_indices[:, 1] < R - 1).nonzero().squeeze(1)[:448]])
    bits = lambda x: x.contiguous().view(torch.int32) if x.dtype == torch.float32 else x
    res["a_equals_b"] = all(bool(torch.equal(bits(x), bits(y))) for x, y in zip(ds.batch(first), comp.batch(first)))
    res["windows_crossing_t0_in_the_check"] = int((ds.valid_indices[first, 1] < R - 1).sum())

    a_us, b_us = [], []
    for _ in range(args.runs):
        a_us.append(timed(ds.batch, pool, args.batches))
        b_us.append(timed(comp.batch, pool, args.batches))
    res.update(a=summary(a_us), b=summary(b_us))
    res["b_over_a"] = res["b"]["median"] / res["a"]["median"]
    # (a)'s algorithmic bytes: the padding is written but not read
    pad_rows = sum(int((R - 1 - ds.valid_indices[s, 1]).clamp(min=0).sum()) for s in pool) / POOL
    per_row = D * 4 + (A - 1) + 200
    nbytes = B * (R * per_row + P * 12 + 16) + (B * R - pad_rows) * per_row + B * (P * 12 + 16 + 8)
    res.update(a_bytes_per_batch=nbytes, a_achieved_GBps=nbytes / (res["a"]["median"] * 1e-6) / 1e9,
               a_frac_of_copy_ceiling=nbytes / (res["a"]["median"] * 1e-6) / COPY_CEILING)

    # the sweep: every variant once per run, so that the variants alternate
    splits = (1, 2, 4, 8, 16)
    sweep = {"split%d" % k: [] for k in splits}
    for _ in range(args.runs):
        for k in splits:
            os.environ["GPUDRIVE_IL_SPLIT"] = str(k)
            sweep["split%d" % k].append(timed(ds.batch, pool, args.batches))
    os.environ.pop("GPUDRIVE_IL_SPLIT", None)
    res["sweep"] = {k: summary(v) for k, v in sweep.items()}
    res["bad_indices"] = int(ds.bad_indices)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    with torch.cuda.stream(torch.cuda.Stream()):  # (the step graph is captured on a stream of torch's own, as in bench.py)
        main()
