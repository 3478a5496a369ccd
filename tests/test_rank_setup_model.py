"""The set-up around k_knn_rank on the host (csrc/rank_cand.hpp cp_threshold, deal_block; tests/rank_setup_model.cpp).

Rows: the checkpoint row of an agent bounded by its own checkpoints, as k_knn_scan's loop builds it, against the row the 64
lanes of the ranking wave build (the shared threshold rule per lane, the first roads' running maximum as the wave's max-scan,
nothing behind the last checkpoint), bit for bit: 1, 2, 39 and 40 checkpoints; first roads increasing, non-monotone, equal, near
65535 and with the 16-bit image of NO_CP; K-th keys of 0, a denormal, 1e30, +inf, NaN and a negative value at the first, the
second, a middle, the last but one and the last checkpoint; `move` of 0, 5.999 and 6; three margins.

The deal: deal_block is a bijection of [0, grid) that maps every aligned group of 8 onto itself and is the identity on a last
partial group, and deal_list (the list of a world: what k_knn_scan uses) is its inverse, for grids 1..130, 1000, 1024, 1025 and 4096; at 1024 and 4096 workgroups with worlds tiled with periods 8 and 16
every XCD list gets exactly the even share of every scene; for every period 1..128 and every scene, that scene 50 % dearer than
the others, the fullest list is at most 1.08 times the mean one (the identity deal: 1.41 at period 8)."""
import os
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
LINES = {("rows", "own_checkpoints"), ("deal", "bijection_groups"), ("share", "even_per_scene"), ("load", "dealt"), ("load", "identity")}


def _binary():
    out = os.path.join(tempfile.gettempdir(), "gd_rank_setup_model_%d" % os.getuid())
    srcs = [os.path.join(HERE, "rank_setup_model.cpp"), os.path.join(HERE, "..", "gpudrive_lab_amd", "csrc", "rank_cand.hpp")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", out, srcs[0]])
    return out


def test_rows_and_deal():
    res = subprocess.run([_binary()], stdout=subprocess.PIPE, universal_newlines=True)
    print(res.stdout)
    got = {}
    for line in res.stdout.splitlines():
        f = line.split()
        if len(f) >= 6 and (f[0], f[1]) in LINES:
            got[(f[0], f[1])] = {f[k]: int(f[k + 1]) for k in range(2, len(f) - 1, 2)}
    assert set(got) == LINES, res.stdout
    for key, r in got.items():
        n = r.get("cases", r.get("grids"))
        assert n > 0, (key, r)
        assert r["bad"] == 0, "%s %s: %d of %d cases fail" % (key[0], key[1], r["bad"], n)
    assert got[("rows", "own_checkpoints")]["cases"] >= 4 * 3 * 6 * 3  # every count, move, key and first-road pattern
    assert got[("deal", "bijection_groups")]["grids"] == 134
    assert got[("load", "dealt")]["worst_milli"] <= 1080
    assert got[("load", "identity")]["worst_milli"] >= 1400  # what the deal removes
    assert res.returncode == 0
