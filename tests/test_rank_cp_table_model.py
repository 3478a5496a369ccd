"""k_knn_rank's table of checkpoints per 32-road chunk on the host: csrc/rank_cand.hpp cp_table (the rule) and the kernel's way
of building it (a max per checkpoint, a running maximum per lane, a max-scan across the lanes) against cp_count and
cp_in_force + 1 for every chunk of the world, then the cull and the scan run with that table against the cull that counts the
checkpoints per block.

tests/rank_cp_table_model.cpp covers rows without a checkpoint, with all 40, with repeated first roads, with several
checkpoints in one chunk, with a first road of 0, with first roads at and beyond the last chunk, rows made non-decreasing by
the running maximum, and values that are no multiples of 32; worlds of 200, 201, 207, 208, 209, 1024, 1025, 1271..1273, 4096 and
10,000 roads (a partial last block, a partial last chunk, an exact multiple of 64 blocks).  Survivor and candidate lists, on
random-walk polylines, an inward spiral with a checkpoint in every chunk and all roads at one point, must be equal element for
element, no dropped block may hold a candidate, and no pass of the scan's unclamped main loop may reach beyond the world."""
import os
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
TABLES = {"none", "all_forty", "repeats", "one_chunk", "first_zero", "at_and_beyond_end", "out_of_order", "any_value"}
LISTS = {"random_walk", "spiral", "one_point"}


def _binary():
    out = os.path.join(tempfile.gettempdir(), "gd_rank_cp_table_model_%d" % os.getuid())
    srcs = [os.path.join(HERE, "rank_cp_table_model.cpp"), os.path.join(HERE, "..", "gpudrive_lab_amd", "csrc", "rank_cand.hpp")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", out, srcs[0]])
    return out


def test_table_is_cp_count_and_the_lists_do_not_change():
    res = subprocess.run([_binary(), "12"], stdout=subprocess.PIPE, universal_newlines=True)
    print(res.stdout)
    tables, lists = {}, {}
    for line in res.stdout.splitlines():
        f = line.split()
        if len(f) == 6 and f[0] == "table":
            tables[f[1]] = {f[k]: int(f[k + 1]) for k in range(2, 6, 2)}
        if len(f) == 14 and f[0] == "lists":
            lists[f[1]] = {f[k]: int(f[k + 1]) for k in range(2, 14, 2)}
    assert set(tables) == TABLES and set(lists) == LISTS, res.stdout
    for name, r in tables.items():
        assert r["rows"] > 0, (name, r)
        assert r["bad"] == 0, "%s: the table differs from cp_count / cp_in_force + 1 for %d of %d rows" % (name, r["bad"], r["rows"])
    for name, r in lists.items():
        assert r["agents"] > 0 and r["cands"] >= 200 * r["agents"] and r["survivors"] >= 13 * r["agents"], (name, r)
        assert r["bad"] == 0, "%s: survivor or candidate list differs for %d of %d agents" % (name, r["bad"], r["agents"])
        assert r["dropped_with_cand"] == 0, "%s: %d dropped blocks hold a candidate" % (name, r["dropped_with_cand"])
        assert r["unclamped_beyond_world"] == 0, "%s: %d roads beyond the world in passes without a clamp" % (name, r["unclamped_beyond_world"])
    assert res.returncode == 0
