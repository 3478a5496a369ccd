#!/usr/bin/env python3
"""The PPO rollout layer at ppo_default (Waymo tiles, 1024 worlds x 128 slots), two ways in one process, one JSON line:

  (a) DeviceRollout: `store` per step (plain and streaming stores), `sort_training_data` + `compute_gae` per rollout (and the
      worst case of a batch without dones), `minibatch` per call (1, 2 and 4 workgroups per sample), `flatten_batch`;
  (b) the best composition in torch alone: per step `mask.nonzero()` -- which is a host synchronisation, the slice to the
      room left needs the count -- and indexed copies; per rollout a device argsort of row * 2^32 + step, the three sorted
      arrays copied to the host and the serial GAE loop there (compiled C, as the reference's c_gae is compiled), and
      `obs[idx]` for a minibatch and for the flattened batch.

Both are fed the same tensors of the same DeviceLearnerEnv rollouts, and (b) is checked equal to (a) before anything is
timed.  Device events around every call; the variants alternate within a step and the order rotates; --runs rollouts, medians
over the steps of a rollout, then median and range over the rollouts.  Bytes are the algorithmic ones (every stored or
gathered observation row read once and written once) against the 6.29 TB/s copy ceiling.
tools/rollout_bench.py [--worlds 1024] [--batch-size 131072] [--minibatch-size 8192] [--runs 3] [--init-steps 0] [--out F]"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from gpudrive_lab_amd.learner import DeviceLearnerEnv, action_table  # noqa: E402
from gpudrive_lab_amd.rollout import DeviceRollout  # noqa: E402

WORKLOAD = "ppo_default"
CEILING = 6.29e12  # bytes / s, the measured copy ceiling
GAMMA, LAMBDA = 0.99, 0.95


def serial_gae_lib():
    d = tempfile.mkdtemp(prefix="gd_rollout_bench_")
    src, so = os.path.join(ROOT, "tools", "serial_gae.c"), os.path.join(d, "serial_gae.so")
    subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, src])
    L = ctypes.CDLL(so)
    fp = ctypes.POINTER(ctypes.c_float)
    L.serial_gae.argtypes = [ctypes.c_int, ctypes.c_float, ctypes.c_float, fp, fp, fp, fp]
    L.serial_gae.restype = None
    return L


class TorchRollout:
    """(b): the same layer in torch alone."""

    def __init__(self, B, mbs, obs_width, L):
        z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device="cuda")  # noqa: E731
        self.B, self.mbs, self.L = B, mbs, L
        self.obs, self.actions = z(B, obs_width), z(B, dt=torch.int64)
        self.logprobs, self.rewards, self.dones, self.values = z(B), z(B), z(B), z(B)
        self.rows, self.steps = z(B, dt=torch.int64), z(B, dt=torch.int64)
        self.ptr = self.step = 0

    def store(self, obs, value, action, logprob, reward, done, mask):
        idx = mask.nonzero().squeeze(1)[: self.B - self.ptr]  # the host synchronisation: nonzero's size
        p, e = self.ptr, self.ptr + int(idx.numel())
        self.obs[p:e] = obs[idx]
        self.values[p:e] = value.view(-1)[idx]
        self.actions[p:e] = action[idx]
        self.logprobs[p:e] = logprob[idx]
        self.rewards[p:e] = reward[idx]
        self.dones[p:e] = done[idx].float()
        self.rows[p:e] = idx
        self.steps[p:e] = self.step
        self.ptr, self.step = e, self.step + 1

    def sort_and_gae(self):
        self.idxs = torch.argsort(self.rows * (1 << 32) + self.steps)
        self.ptr = self.step = 0
        d, v, r = (x[self.idxs].cpu().numpy() for x in (self.dones, self.values, self.rewards))
        adv = np.empty_like(d)
        fp = ctypes.POINTER(ctypes.c_float)
        self.L.serial_gae(len(d), GAMMA, LAMBDA, *(a.ctypes.data_as(fp) for a in (d, v, r, adv)))
        self.advantages = torch.from_numpy(adv).cuda()
        return self.idxs, self.advantages

    def minibatch(self, mb):
        nm = self.B // self.mbs
        p = self.idxs.view(self.mbs, nm)[:, mb]
        a = self.advantages.view(self.mbs, nm)[:, mb].contiguous()
        v = self.values[p]
        return (self.obs[p].unsqueeze(1), self.actions[p].unsqueeze(1), self.logprobs[p].unsqueeze(1),
                self.dones[p].unsqueeze(1), v, a, a + v)

    def flatten_batch(self):
        nm = self.B // self.mbs
        b = self.idxs.view(self.mbs, nm).t().contiguous()
        a = self.advantages.view(self.mbs, nm).t().contiguous()
        v = self.values[b]
        return (self.obs[b].unsqueeze(2), self.actions[b].unsqueeze(2), self.logprobs[b].unsqueeze(2),
                self.dones[b].unsqueeze(2), v, a, a + v)


def ev():
    return torch.cuda.Event(enable_timing=True)


def timed_call(fn):
    e0, e1 = ev(), ev()
    e0.record()
    out = fn()
    e1.record()
    return (e0, e1), out


def ms(pair):
    return pair[0].elapsed_time(pair[1])


def med_range(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), n=len(xs))


def equal(a, b):
    return a.shape == b.shape and bool((a.contiguous().view(torch.uint8) == b.contiguous().view(torch.uint8)).all())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worlds", type=int, default=1024)
    ap.add_argument("--batch-size", type=int, default=131072)
    ap.add_argument("--minibatch-size", type=int, default=8192)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--init-steps", type=int, default=0)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    B, mbs = args.batch_size, args.minibatch_size
    kw = bench.params_for(WORKLOAD)
    _, order, agents = bench.split_workload(WORKLOAD)
    scenes = bench.scenes_for(WORKLOAD, args.worlds, 0, agents=agents)
    sim = bench.make_sim(scenes, kw, agents, 0, knn_order=order)
    env = DeviceLearnerEnv(sim, init_steps=args.init_steps)
    N, D = env.num_agents, int(env.obs.shape[1])
    table = action_table("classic").cuda()
    gen = torch.Generator(device="cuda").manual_seed(0)
    res = dict(tool="tools/rollout_bench.py", workload=WORKLOAD, worlds=args.worlds, rows=N, obs_width=D, batch_size=B,
               minibatch_size=mbs, bptt_horizon=1, runs=args.runs, init_steps=args.init_steps, source_stamp=bench.source_stamp())

    ro = DeviceRollout(B, mbs, 1, num_rows=N, obs_width=D)
    ro_nt = DeviceRollout(B, mbs, 1, num_rows=N, obs_width=D, streaming_stores=True)
    tb = TorchRollout(B, mbs, D, serial_gae_lib())
    res["a_nbytes"] = ro.nbytes
    obs = env.reset()
    obs, rewards, terminals, _, masks = env.step(torch.randint(0, table.shape[0], (N,), device="cuda", generator=gen))
    out_a = None
    runs = {k: [] for k in ("a_store", "a_store_streaming", "b_store", "env_step", "a_sort_gae", "b_sort_gae", "a_minibatch",
                            "a_minibatch_split2", "a_minibatch_split4", "b_minibatch", "a_flatten", "b_flatten", "live_rows",
                            "steps")}
    for run in range(args.runs + 1):  # rollout 0 is the warm-up and the equality check
        pairs = {k: [] for k in ("a_store", "a_store_streaming", "b_store", "env_step")}
        live, step = [], 0
        while not ro.full:
            action = torch.randint(0, table.shape[0], (N,), device="cuda", generator=gen)
            value, logprob = obs[:, 0] * 0.5 + obs[:, 1], -(obs[:, 2].abs())
            inputs = (obs, value, action, logprob, rewards, terminals, masks)
            variants = [("a_store", ro), ("a_store_streaming", ro_nt), ("b_store", tb)]
            k = (step + run) % 3
            for name, r in variants[k:] + variants[:k]:
                pairs[name].append(timed_call(lambda: r.store(*inputs))[0])
            live.append(masks.sum())
            p, (obs, rewards, terminals, _, masks) = timed_call(lambda: env.step(action))
            pairs["env_step"].append(p)
            step += 1
        torch.cuda.synchronize()
        assert tb.ptr == B and ro_nt.full
        sort_order = [("a", lambda: (ro.sort_training_data(), ro.compute_gae(GAMMA, LAMBDA))), ("b", tb.sort_and_gae)]
        if run % 2:
            sort_order.reverse()
        sort_pairs = {}
        for name, fn in sort_order:
            sort_pairs[name], _ = timed_call(fn)
        ro_nt.sort_training_data()
        torch.cuda.synchronize()
        if run == 0:
            for name in ("obs", "actions", "logprobs", "rewards", "dones", "values"):
                assert equal(getattr(ro, name), getattr(tb, name)), name
                assert equal(getattr(ro, name), getattr(ro_nt, name)), name + " (streaming)"
            assert torch.equal(ro.idxs, tb.idxs)
            assert bool((ro.advantages == tb.advantages).all()), "advantages"
        if out_a is None:
            out_a = ro.minibatch(0)
        nm = ro.num_minibatches
        mb_pairs = {k: [] for k in ("a_minibatch", "a_minibatch_split2", "a_minibatch_split4", "b_minibatch")}
        for mb in range(nm):
            calls = [("a_minibatch", lambda: ro._gather(mb, 1, out_a, 1)), ("a_minibatch_split2", lambda: ro._gather(mb, 1, out_a, 2)),
                     ("a_minibatch_split4", lambda: ro._gather(mb, 1, out_a, 4)), ("b_minibatch", lambda: tb.minibatch(mb))]
            k = (mb + run) % 4
            for name, fn in calls[k:] + calls[:k]:
                p, out = timed_call(fn)
                mb_pairs[name].append(p)
                if run == 0 and name != "b_minibatch":
                    want = tb.minibatch(mb)
                    assert all(equal(x, y) for x, y in zip(out, want)), (name, mb)
        fa, flat_a = timed_call(ro.flatten_batch)
        fb, flat_b = timed_call(tb.flatten_batch)
        torch.cuda.synchronize()
        if run == 0:
            assert all(equal(x, y) for x, y in zip(flat_a, flat_b)), "flatten_batch"
            assert int(ro.bad_positions.item()) == 0
        del flat_a, flat_b
        ro.b_obs = None
        torch.cuda.empty_cache()
        if run == 0:
            continue
        for k, ps in pairs.items():
            runs[k].append(statistics.median(ms(p) for p in ps))
        runs["a_sort_gae"].append(ms(sort_pairs["a"]))
        runs["b_sort_gae"].append(ms(sort_pairs["b"]))
        for k, ps in mb_pairs.items():
            runs[k].append(statistics.median(ms(p) for p in ps))
        runs["a_flatten"].append(ms(fa))
        runs["b_flatten"].append(ms(fb))
        runs["live_rows"].append(float(torch.stack(live).float().mean().item()))
        runs["steps"].append(step)

    # the worst case: no done in the batch, one chain of B (the storage of the last rollout, its dones cleared)
    ro.dones.zero_()
    worst = []
    for _ in range(args.runs):
        p, _ = timed_call(lambda: ro.compute_gae(GAMMA, LAMBDA))
        torch.cuda.synchronize()
        worst.append(ms(p))
    res["ms"] = {k: med_range(v) for k, v in runs.items()}
    res["ms"]["a_gae_no_dones"] = med_range(worst)
    m = {k: v["median"] for k, v in res["ms"].items()}
    res["b_over_a"] = dict(store=m["b_store"] / m["a_store"], sort_gae=m["b_sort_gae"] / m["a_sort_gae"],
                           minibatch=m["b_minibatch"] / m["a_minibatch"], flatten=m["b_flatten"] / m["a_flatten"])
    copy_bytes = 2 * m["live_rows"] * D * 4
    gather_bytes = 2 * mbs * D * 4
    res["bytes"] = dict(store_copy=copy_bytes, minibatch=gather_bytes, flatten=2 * B * D * 4)
    res["ceiling_fraction"] = dict(a_store=copy_bytes / (m["a_store"] * 1e-3) / CEILING,
                                   a_store_streaming=copy_bytes / (m["a_store_streaming"] * 1e-3) / CEILING,
                                   a_minibatch=gather_bytes / (m["a_minibatch"] * 1e-3) / CEILING,
                                   a_flatten=2 * B * D * 4 / (m["a_flatten"] * 1e-3) / CEILING)
    res["host_reads_per_rollout"] = ro.host_reads / (args.runs + 1)
    sim.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    with torch.cuda.stream(torch.cuda.Stream()):  # (the step graph is captured on a stream of torch's own, as in bench.py)
        main()
