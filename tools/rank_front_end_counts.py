#!/usr/bin/env python3
"""developer tool: the candidate counts of tests/test_gpu_rank_front_end.py's worlds (debug_road_path() after every selection) as
a given build of the library produces them.

  tools/rank_front_end_counts.py <library.so> --out <file.json>   run the cases on that build and write the counts
  tools/rank_front_end_counts.py <library.so> --check             run them and compare with tests/golden/rank_front_end_counts.json

The golden file is recorded from the build BEFORE a change of k_knn_rank's front end (tools/build_expt.sh <name> on that commit,
then --out) and checked on the build after it: the candidate set must not move, not even to another superset.  The cases run
through pytest in a child process, so the counts are taken exactly where the test takes them."""
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "rank_front_end_counts.json")


def main(argv):
    if len(argv) < 3 or argv[2] not in ("--out", "--check") or (argv[2] == "--out" and len(argv) < 4):
        print(__doc__)
        return 2
    lib = os.path.abspath(argv[1])
    out = os.path.abspath(argv[3]) if argv[2] == "--out" else os.path.join(tempfile.mkdtemp(), "counts.json")
    if os.path.exists(out):
        os.remove(out)
    env = dict(os.environ, GPUDRIVE_DEV="1", GPUDRIVE_AMD_LIB=lib, GPUDRIVE_RANK_FRONT_END_RECORD=out)
    res = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", os.path.join(ROOT, "tests", "test_gpu_rank_front_end.py")],
                         cwd=ROOT, env=env)
    if res.returncode != 0:
        print("the cases did not pass on %s" % lib)
        return 1
    got = json.load(open(out))
    print("%s: %s" % (lib, {k: [sum(c) for c in v] for k, v in got.items()}))
    if argv[2] == "--check":
        want = json.load(open(GOLDEN))
        diff = sorted(k for k in set(got) | set(want) if got.get(k) != want.get(k))
        print("counts equal to %s: %s" % (os.path.relpath(GOLDEN, ROOT), "yes" if not diff else "NO: %s" % diff))
        return 0 if not diff else 1
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
