"""k_knn_replay's prologue on the host: csrc/rank_heap.hpp (the code the kernel runs) against std::make_heap with the rank
comparator and against the plain slot-by-slot fill, for both rank formats (tie field of 5 and of 4 bits).

tests/replay_heap_model.cpp generates the inputs: 10,000 random tie-free arrays of 200 ranks (run through the tie-free form
and the one for equal keys), 10,000 with several groups of equal keys, 1,000 drawn from a handful of keys, all-equal, sorted
and reverse-sorted arrays (with and without equal neighbours).  Every one of the 200 slots must equal libstdc++'s, slot 0,
slot 201 and the pairs beyond the heap must still be 0, and no access may leave the 128 pairs of a column."""
import os
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))


def _binary():
    out = os.path.join(tempfile.gettempdir(), "gd_replay_heap_model_%d" % os.getuid())
    srcs = [os.path.join(HERE, "replay_heap_model.cpp"), os.path.join(HERE, "..", "gpudrive_lab_amd", "csrc", "rank_heap.hpp")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", out, srcs[0]])
    return out


def test_rank_heap_prologue_equals_std_make_heap_and_the_plain_fill():
    res = subprocess.run([_binary(), "10000"], stdout=subprocess.PIPE, universal_newlines=True)
    print(res.stdout)
    rows = {}
    for line in res.stdout.splitlines():
        f = line.split()
        if len(f) == 7:
            rows[f[0]] = (int(f[2]), int(f[4]), int(f[6]))
    assert set(rows) == {"distinct", "equal_groups", "few_keys", "all_equal", "sorted", "reverse_sorted"}, res.stdout
    assert rows["distinct"][0] >= 20000 and rows["equal_groups"][0] >= 20000 and rows["few_keys"][0] >= 2000
    assert rows["all_equal"][0] == 2 and rows["sorted"][0] == 4 and rows["reverse_sorted"][0] == 4
    for name, (cases, bad, fill_bad) in rows.items():
        assert bad == 0, "%s: make_heap differs from std::make_heap in %d of %d arrays" % (name, bad, cases)
        assert fill_bad == 0, "%s: the pair fill differs from the slot-by-slot fill in %d of %d arrays" % (name, fill_bad, cases)
    assert "bad_access 0" in res.stdout
    assert res.returncode == 0
