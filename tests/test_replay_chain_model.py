"""The registers k_knn_replay keeps across its rounds, on the host: csrc/rank_heap.hpp (the code the kernel runs) with the
chain mirrors `q` -- slots 12, 25, 50, 100, the ancestors of slot K that a round no longer reads back from the column -- held
across every round, block and change of form, against the reference algorithm on keys (std::make_heap, then per candidate
`key < heap[0]`, std::pop_heap, replace last, std::push_heap with the strict key comparator).

tests/replay_chain_model.cpp runs model waves of four lanes, both rank formats (tie field of 5 bits / up to 1272 candidates and
4 bits / up to 2552), the input families of tests/replay_rounds_model.cpp and a wave of one agent beside idle lanes, and the
kernel's choice of form per block.  After EVERY round it asserts that the mirrors equal the column's slots (`mirror_bad`), that
the whole heap array and the root equal the reference's, that a round inserts exactly when the reference does and that the
slots that must hold 0 do (`bad`); that a round of the checked form told to step back leaves r, last, q and the column
untouched (`inv_bad`); after every block, that the overloads with mirrors and the signatures without them (which load the
mirrors from the column per call) give the same column, r, last and tie track (`wrap_bad`).  `via12` .. `via100` count the
inserts whose pop path, followed on the reference's keys, passes through a mirrored slot: the rounds in which the pop patches
a mirror.  A family that never does so has tested nothing and fails.

The same program is built with -fsanitize=address,undefined and run stand-alone on fewer waves."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
KINDS = {"tie_free", "random_groups", "meet_at_root", "stay_to_end", "after_eviction", "fails_entry", "inside_first_k", "all_equal",
         "idle_lanes"}
FIELDS = 29  # name + 14 (label, value) pairs
WAVES = 40
WAVES_SANITIZED = 6


def _binary(directory, tag, flags):
    out = os.path.join(str(directory), "replay_chain_model_%s" % tag)
    subprocess.check_call(["g++", "-std=c++17"] + flags + ["-o", out, os.path.join(HERE, "replay_chain_model.cpp")])
    return out


def _run(binary, waves):
    res = subprocess.run([binary, str(waves)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    print(res.stdout)
    print(res.stderr)
    rows = {}
    for line in res.stdout.splitlines():
        f = line.split()
        if len(f) == FIELDS:
            rows[f[0]] = {f[k]: int(f[k + 1]) for k in range(1, FIELDS, 2)}
    assert set(rows) == KINDS, res.stdout
    for name, r in rows.items():
        assert r["waves"] == waves, name
        assert r["bad"] == 0, "%s: heap, root, inserts or zero slots differ from the reference's in %d of %d waves" % (name, r["bad"], waves)
        assert r["mirror_bad"] == 0, "%s: a mirror differs from its slot of the column in %d of %d waves" % (name, r["mirror_bad"], waves)
        assert r["inv_bad"] == 0, "%s: a checked round that stepped back changed the lane in %d of %d waves" % (name, r["inv_bad"], waves)
        assert r["wrap_bad"] == 0, "%s: rounds with and without held mirrors differ in %d of %d waves" % (name, r["wrap_bad"], waves)
        assert r["inserts"] > 0 and r["rounds"] >= r["inserts"], (name, r)
        for slot in ("via12", "via25", "via50", "via100"):
            assert r[slot] > 0, "%s: the pop's path never passed through slot %s" % (name, slot[3:])
    for name in ("tie_free", "idle_lanes"):
        assert rows[name]["ties_blocks"] == 0 and rows[name]["checked_blocks"] == 0, "a wave without equal keys left the plain form"
    for name in KINDS - {"tie_free", "idle_lanes"}:  # every form ran, and rounds of the checked form went both ways
        r = rows[name]
        assert r["ties_blocks"] > 0 and r["checked_blocks"] > 0 and r["stepped_back"] > 0, (name, r)
    assert "bad_access 0" in res.stdout
    assert res.returncode == 0, res.stderr
    return rows


def test_chain_mirrors_follow_the_column_after_every_round(tmp_path):
    _run(_binary(tmp_path, "o2", ["-O2"]), WAVES)


def test_chain_model_under_address_and_undefined_sanitizers(tmp_path):
    """the stand-alone program, instrumented: out-of-range slots, shifts and signed overflow in the rounds would stop it"""
    _run(_binary(tmp_path, "san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]), WAVES_SANITIZED)
