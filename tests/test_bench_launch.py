"""`python bench.py --gpus N` must start its own ranks (the driver calls it exactly like that): N child processes through
torch.distributed.run, spawned before anything touches the GPU, rank 0's JSON line forwarded, a failing rank = a failing
exit code.  Runs on the CPU box with gloo and `--dry-run` (no GPU work: the ranks only join the group and are counted)."""
import json
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*args):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], env=env, capture_output=True, text=True,
                          timeout=600)


def test_two_ranks_without_a_launcher():
    r = _run("--gpus", "2", "--dist-backend", "gloo", "--dry-run")
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout  # rank 0 alone prints
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["ranks_counted"] == 2
    assert line["distributed"] == {"world_size": 2, "backend": "gloo"}
    assert "spawning" in r.stderr


def test_a_failing_rank_fails_the_launch():
    if torch.cuda.is_available():
        return  # (on a GPU box the ranks would run the benchmark: covered by the bench itself)
    r = _run("--gpus", "2", "--dist-backend", "gloo", "--steps", "1", "--warmup", "0")
    assert r.returncode != 0
    assert "needs an MI355X" in r.stderr


def test_a_rank_that_leaves_with_an_error_fails_the_launch_with_or_without_a_gpu():
    """The exit-code path of the self-launch on any box: in --dry-run nothing touches a GPU, rank 1 leaves with an error after
    the ranks were counted, and `python bench.py --gpus 2` must not return 0."""
    r = _run("--gpus", "2", "--dist-backend", "gloo", "--dry-run", "--dry-run-fail-rank", "1")
    assert r.returncode != 0, r.stdout[-500:]


def test_eight_ranks_and_one_gather_round_without_a_launcher():
    """The launch the driver makes on an 8-GPU node, rehearsed with gloo on the CPU box: eight ranks counted, one round of
    config 4's observation gather in both modes with unequal controlled counts, every rank's rows in its own section --
    so that the first RCCL run of the class is not also its first 8-rank run."""
    r = _run("--gpus", "8", "--dist-backend", "gloo", "--dry-run")
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
    assert line["n_gpus"] == 8 and line["ranks_counted"] == 8
    assert line["gather_round"]["ok"] is True and len(line["gather_round"]["controlled_per_rank"]) == 8
    t = line["gather_bytes_per_rank"]
    assert t["raw_rows"]["bytes_per_agent"] < t["packed"]["bytes_per_agent"]
    assert t["packed"]["raw"] == 1024 * 64 * 4 * (6 + 63 * 6 + 200 * 13)


def _processes():
    """(pid, argv) of every live process, from /proc."""
    out = []
    for pid in os.listdir("/proc"):
        if pid.isdigit():
            try:
                with open("/proc/%s/cmdline" % pid, "rb") as fh:
                    argv = fh.read().split(b"\0")
                with open("/proc/%s/stat" % pid) as fh:
                    if fh.read().rsplit(")", 1)[1].split()[0] == "Z":
                        continue
                out.append((pid, [a.decode("utf-8", "replace") for a in argv]))
            except OSError:
                pass
    return out


def test_a_signal_to_the_launcher_ends_every_rank():
    """`timeout` around bench.py (tools, the driver) signals only the parent: the ranks live in a session of their own and must
    be ended with it, not left on the GPUs."""
    import signal
    import time
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    p = subprocess.Popen([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dist-backend", "gloo", "--dry-run",
                          "--dry-run-sleep", "120"], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    deadline = time.time() + 120
    kids = []
    while time.time() < deadline and len(kids) < 3:   # the launcher (torch.distributed.run) and its two ranks (which it starts in
        time.sleep(1.0)                               # sessions of their own and ends when it is told to end)
        kids = [pid for pid, cmd in _processes()
                if "--dry-run-sleep" in cmd and pid != str(p.pid) and ("torch.distributed.run" in cmd or "-u" in cmd)]
    assert len(kids) >= 3, "the ranks did not start: %r %r %s" % (kids, p.poll(), (p.stderr.read()[-800:] if p.poll() is not None else ""))
    time.sleep(3.0)   # (the ranks have joined the group and sleep)
    p.send_signal(signal.SIGTERM)
    p.wait(timeout=60)
    for _ in range(20):
        alive = [pid for pid, _ in _processes()]
        left = [k for k in kids if k in alive]
        if not left:
            break
        time.sleep(1.0)
    assert not left, "ranks survived the launcher"


class _FakeTensor:
    def __init__(self, t):
        self._t = t

    def to_torch(self):
        return self._t


class _FakeSim:
    """The slot getters dump_outputs reads, on host tensors of the exported shapes (W worlds x 64 agent slots)."""

    def __init__(self, worlds):
        g = torch.Generator().manual_seed(3)
        W, A = worlds, 64
        self.t = dict(reward=torch.rand(W, A, 1, generator=g), done=torch.randint(0, 2, (W, A, 1), generator=g, dtype=torch.int32),
                      info=torch.randint(-3, 3, (W, A, 5), generator=g, dtype=torch.int32),
                      self_observation=torch.rand(W, A, 8, generator=g), absolute_self_observation=torch.rand(W, A, 14, generator=g),
                      steps_remaining=torch.randint(0, 91, (W, A, 1), generator=g, dtype=torch.int32),
                      partner_observations=torch.rand(W, A, A - 1, 9, generator=g), agent_roadmap=torch.rand(W, A, 200, 9, generator=g))

    def __getattr__(self, name):
        if name.endswith("_tensor") and name[:-len("_tensor")] in self.__dict__.get("t", {}):
            return lambda: _FakeTensor(self.t[name[:-len("_tensor")]])
        raise AttributeError(name)


def test_dump_outputs_writes_a_fixed_sample_within_the_byte_budget(tmp_path, monkeypatch):
    """--dump-outputs: one .npy per array the step hands its caller, floats as float32 and ints as float64 (exact), the
    same seeded sample of worlds in every run when everything would exceed the budget, and never more bytes than it."""
    import numpy as np
    before = set(os.environ)
    import bench
    for k in set(os.environ) - before:  # (bench.py's environment defaults are for its own process)
        del os.environ[k]
    sim = _FakeSim(40)
    monkeypatch.setattr(bench, "DUMP_BYTES", 4 << 20)
    kw = bench.params_for("synthetic")
    a = bench.dump_outputs(sim, str(tmp_path / "a"), "synthetic", kw)
    b = bench.dump_outputs(sim, str(tmp_path / "b"), "synthetic", kw)
    assert a["worlds"] == b["worlds"] and a["worlds"] != "all" and 0 < len(a["worlds"]) < 40
    assert a["bytes"] <= 4 << 20
    assert sorted(os.listdir(tmp_path / "a")) == a["files"] == sorted(k + ".npy" for k in sim.t)
    idx = a["worlds"]
    for k, t in sim.t.items():
        arr = np.load(tmp_path / "a" / (k + ".npy"))
        assert arr.dtype == (np.float32 if t.is_floating_point() else np.float64), k
        assert np.array_equal(arr, t[idx].numpy().astype(arr.dtype)), k
        assert np.array_equal(arr, np.load(tmp_path / "b" / (k + ".npy"))), k
    # (the raw partner / road rows are left out where the step does not write them)
    c = bench.dump_outputs(sim, str(tmp_path / "c"), "synthetic", kw, raw_rows=False)
    assert "agent_roadmap.npy" not in c["files"] and c["worlds"] == "all"


@pytest.mark.gpu
def test_dumped_outputs_do_not_depend_on_the_spin_up(tmp_path):
    """Two runs of the same timed steps, one with no spin-up and one with 200 ms of it (a different number of untimed steps
    before the stretch), must dump the same arrays bit for bit; `--steps` sets the number of timed steps."""
    import numpy as np
    lines = []
    for spin, d in (("0", "a"), ("200", "b")):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "3",
                            "--full", "--workloads", "synthetic", "--worlds", "64", "--no-cpu-baseline", "--spin-ms", spin,
                            "--dump-outputs", str(tmp_path / d)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        lines.append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]))
    for line in lines:
        assert line["steps"] == 7 and line["ms_per_step"] > 0
        assert line["kernels"]["k_world_step"]["launches"] == 7
    a, b = (line["dump_outputs"] for line in lines)
    assert a["files"] == b["files"] and "agent_roadmap.npy" in a["files"] and a["bytes"] <= 64 << 20
    for f in a["files"]:
        x, y = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert x.dtype in (np.float32, np.float64) and x.shape[0] == 64
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), f


def test_every_run_writes_the_scenes_it_times_and_removes_them():
    """No run reads what an earlier run left behind: each process writes the synthetic scenes into a directory of its own,
    which is gone when it exits."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    code = "import bench; p = bench.scenes_for('synthetic', 16, 0); print(p[0]); print(len(set(p)))"
    seen = []
    for _ in range(2):
        r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        path, distinct = r.stdout.split()[-2:]
        assert int(distinct) == 8 and path.endswith(".json")
        assert not os.path.exists(os.path.dirname(path)), path
        seen.append(path)
    assert seen[0] != seen[1]


@pytest.mark.gpu
def test_a_plain_run_times_the_primary_workload_alone_and_dumps_what_a_full_run_dumps(tmp_path):
    """Without --full a run times the primary workload and nothing else: its line has the headline figure and none of the
    kernel times, rooflines, other workloads or CPU baseline that --full adds, and --dump-outputs writes the same arrays,
    bit for bit, as a --full run with the same arguments."""
    import numpy as np
    lines = {}
    for mode, extra in (("plain", []), ("full", ["--full", "--workloads", "synthetic", "--no-cpu-baseline"])):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "3",
                            "--worlds", "64", "--dump-outputs", str(tmp_path / mode), *extra],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        lines[mode] = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    plain, full = lines["plain"], lines["full"]
    assert plain["full"] is False and full["full"] is True
    for k in ("metric", "unit", "higher_is_better", "dtype", "steps", "warmup", "n_gpus", "config"):
        assert plain[k] == full[k], k
    assert plain["steps"] == 7 and plain["ms_per_step"] > 0 and plain["value"] > 0
    assert plain["other_workloads"] == [] and plain["engine"]["rank_audit_violations"] == 0
    for k in ("ms_per_step_events", "kernels", "roofline", "other_rooflines", "cpu_baseline", "allgather"):
        assert k not in plain and k in full, k
    assert full["kernels"]["k_world_step"]["launches"] == 7
    a, b = plain["dump_outputs"], full["dump_outputs"]
    assert a["files"] == b["files"] and a["worlds"] == b["worlds"]
    for f in a["files"]:
        x, y = np.load(tmp_path / "plain" / f), np.load(tmp_path / "full" / f)
        assert x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8)), f
