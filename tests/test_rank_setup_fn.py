"""The per-lane decision of the rank path's set-up on the host (csrc/rank_setup.hpp decide; tests/rank_setup_fn_model.cpp).

k_world_step's FOLD instantiations and the thin k_knn_scan run one text, rank_setup::run, whose decision per agent -- too far from
every road, fallback or bypass, bounded afresh, by its own checkpoints (which set, `move`, `margin`, the 16-byte record) or by a
donor's -- is plain C++.  The program restates the expressions of the kernel that text was taken out of and compares the two bit
for bit over 7,500 seeded cases in five families: ordinary steps (every agent on its own checkpoints), road boxes at distances
around the far test's limit, neighbours within reach of an agent that lost its own bound (donors, a NaN header among them),
stored quaternions off the unit circle (the margin), and GPUDRIVE_RANK_SCAN_ROWS (every agent a row).  Distances of exactly
0, 5.999, 6 and 6.0001 m to a header, 0, -1, 1, 39 and 40 checkpoints, road counts at K - 1, K, rk_min_roads - 1, rk_min_roads,
the largest world and one more.  Built once plain and once with AddressSanitizer and UBSan (the header's loops over the 64
published headers)."""
import os
import subprocess
import tempfile

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "gpudrive_lab_amd", "csrc")
FAMILIES = {"ordinary_step": 1500, "far_test": 1500, "donors": 2000, "stored_quaternions": 1500, "every_row": 1000}


def _binary(tag, flags):
    out = os.path.join(tempfile.gettempdir(), "gd_rank_setup_fn_%s_%d" % (tag, os.getuid()))
    srcs = [os.path.join(HERE, "rank_setup_fn_model.cpp"), os.path.join(CSRC, "rank_setup.hpp"), os.path.join(CSRC, "rank_cand.hpp")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas"] + flags + ["-o", out, srcs[0]])
    return out


@pytest.mark.parametrize("tag,flags", [("plain", []), ("san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])])
def test_decision_matches_the_former_kernel(tag, flags):
    res = subprocess.run([_binary(tag, flags)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    print(res.stdout)
    got = {}
    for line in res.stdout.splitlines():
        f = line.split()
        if len(f) >= 6 and f[0] == "decide":
            got[f[1]] = {f[k]: int(f[k + 1]) for k in range(2, len(f) - 1, 2)}
    assert set(got) == set(FAMILIES), res.stdout
    for name, r in got.items():
        assert r["cases"] == FAMILIES[name], (name, r)
        assert r["bad"] == 0, "%s: %d of %d cases differ from the former kernel" % (name, r["bad"], r["cases"])
    # every branch of the decision was reached, each in the family made for it
    assert got["ordinary_step"]["own"] == FAMILIES["ordinary_step"], got["ordinary_step"]
    assert got["far_test"]["far"] > 200 and got["far_test"]["far"] < FAMILIES["far_test"] - 200, got["far_test"]
    assert got["donors"]["row"] > 100 and got["donors"]["afresh"] > 100 and got["donors"]["fallback"] > 100, got["donors"]
    assert got["every_row"]["own"] == 0 and got["every_row"]["row"] > 100, got["every_row"]
    assert res.returncode == 0, res.stdout
