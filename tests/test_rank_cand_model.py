"""k_knn_rank's candidate front end on the host: csrc/rank_cand.hpp (the per-road test, the checkpoint in force, the block test
-- the code the kernel runs) as the kernel uses it, against a plain loop over every road of the world.

tests/rank_cand_model.cpp culls the blocks of 16 consecutive roads a batch of 64 at a time, counting the checkpoints at or before
a block's chunk as the kernel does (two ballots and the entries between them, on the running maximum that k_knn_scan stores),
scans the surviving blocks in index order and compares the candidate list, element for element, with the list of a loop over
all roads that finds the checkpoint in force by the rule of the scan this replaces.  No dropped block may hold a candidate.
Inputs: random-walk polylines like synth.make_scene's, thousands of metres from the origin; a checkpoint at every 32-road chunk;
thresholds of +inf, 0 and tiny ones, first roads repeated and out of order; an inward spiral on which every road is a candidate;
all roads at one point; the agent on a block's centre, on a road, far outside; worlds of K, K + 1, 207, 208, 209, 1271..1273,
4096 and 10,000 roads, so that a partial last block and a partial last chunk both occur."""
import os
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = {"random_walk", "every_chunk", "inf_and_tiny", "spiral", "one_point", "centre_and_far"}


def _binary():
    out = os.path.join(tempfile.gettempdir(), "gd_rank_cand_model_%d" % os.getuid())
    srcs = [os.path.join(HERE, "rank_cand_model.cpp"), os.path.join(HERE, "..", "gpudrive_lab_amd", "csrc", "rank_cand.hpp")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", out, srcs[0]])
    return out


def test_cull_and_ordered_scan_give_the_plain_loops_candidates():
    res = subprocess.run([_binary(), "12"], stdout=subprocess.PIPE, universal_newlines=True)
    print(res.stdout)
    rows = {}
    for line in res.stdout.splitlines():
        f = line.split()
        if len(f) == 15 and f[0] in CASES:
            rows[f[0]] = {f[k]: int(f[k + 1]) for k in range(1, 15, 2)}
    assert set(rows) == CASES, res.stdout
    for name, r in rows.items():
        assert r["agents"] > 0 and r["cands"] >= 200 * r["agents"], (name, r)
        assert r["bad"] == 0, "%s: the candidate list differs from the plain loop's for %d of %d agents" % (name, r["bad"], r["agents"])
        assert r["dropped_with_cand"] == 0, "%s: %d dropped blocks hold a candidate" % (name, r["dropped_with_cand"])
    # the cull does cull (random walks: most blocks go) and the overflow cases occur (more candidates than the ranking holds)
    assert rows["random_walk"]["survivors"] * 2 < rows["random_walk"]["blocks"], rows["random_walk"]
    assert rows["spiral"]["overflow"] > 0 and rows["one_point"]["overflow"] > 0
    assert res.returncode == 0
