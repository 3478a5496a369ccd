"""k_knn_replay's rounds on the host: csrc/rank_heap.hpp (the code the kernel runs) against the reference algorithm on keys
-- std::make_heap, then per candidate `key < heap[0]`, std::pop_heap, replace last, std::push_heap with the strict key
comparator -- for both rank formats (tie field of 5 and of 4 bits) and up to the most candidates each is ranked with.

tests/replay_rounds_model.cpp runs model waves of four lanes.  Per block of eight candidates the wave takes the equal-key form
of the round if any of its lanes has a candidate with a non-zero tie field in the block, the checked form (plain rounds, each
redone in the equal-key form if any inserting lane met a rank with a non-zero tie field) if any lane has such an element in its
heap, and the plain form otherwise, exactly as the kernel's loop decides; the heap array and the root of every lane are compared
with the reference's after every tile of 32 candidates and at the end.  `inv_bad` counts the waves that broke what the forms
rest on: in a plain block no two elements of heap + candidates share a key; a checked round that is told to step back leaves
the lane untouched; a checked round committed in the plain form equals the equal-key form's.  Inputs: tie-free sequences; random groups of 2..12 equal keys; a
group whose members meet at the root; groups that stay to the end; a member that arrives after its group was evicted; a member
that fails the entry test; groups inside the first K; every key shared by as many candidates as a rank can count; always a
lane without ties (and mostly an idle one) beside the tied one.  A wave without equal keys must never leave the plain form,
whatever the slack behind its candidates holds."""
import os
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
KINDS = {"tie_free", "random_groups", "meet_at_root", "stay_to_end", "after_eviction", "fails_entry", "inside_first_k", "all_equal"}
WAVES = 300


def _binary():
    out = os.path.join(tempfile.gettempdir(), "gd_replay_rounds_model_%d" % os.getuid())
    srcs = [os.path.join(HERE, "replay_rounds_model.cpp"), os.path.join(HERE, "..", "gpudrive_lab_amd", "csrc", "rank_heap.hpp")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", out, srcs[0]])
    return out


def test_mixed_form_rounds_equal_the_reference_heap_on_keys():
    res = subprocess.run([_binary(), str(WAVES)], stdout=subprocess.PIPE, universal_newlines=True)
    print(res.stdout)
    rows = {}
    for line in res.stdout.splitlines():
        f = line.split()
        if len(f) == 17:
            rows[f[0]] = {f[k]: int(f[k + 1]) for k in range(1, 17, 2)}
    assert set(rows) == KINDS, res.stdout
    for name, r in rows.items():
        assert r["waves"] == WAVES, name
        assert r["bad"] == 0, "%s: the heap differs from the reference's in %d of %d waves" % (name, r["bad"], r["waves"])
        assert r["inv_bad"] == 0, "%s: a plain block met two elements with one key in %d of %d waves" % (name, r["inv_bad"], r["waves"])
    assert rows["tie_free"]["ties_blocks"] == 0 and rows["tie_free"]["checked_blocks"] == 0, "a wave without equal keys left the plain form"
    for name in KINDS - {"tie_free"}:  # every form was exercised, and rounds of the checked form went both ways
        r = rows[name]
        assert r["ties_blocks"] > 0 and r["checked_blocks"] > 0 and 0 < r["redone"] < r["checked_inserts"], (name, r)
        assert r["ties_blocks"] + r["checked_blocks"] < r["blocks"] or name == "all_equal", (name, r)
    assert "bad_access 0" in res.stdout
    assert res.returncode == 0
