#!/usr/bin/env python3
"""developer tool: k_knn_replay's phase clocks (map_obs_rank.hip ReplayClock, a -DGD_CLOCKS build: tools/build_expt.sh clk -DGD_CLOCKS).
  EXPT=clk python3 tools/replay_clocks.py [synthetic|waymo|cfg3] [steps]
Per step: the phases of the slowest of the first 32 waves (us at the 100 MHz clock), whether it ran the equal-key copy, the
longest total of any wave and of any wave on the equal-key copy, how many waves ran that copy, and the share of those waves'
blocks of eight candidates that ran in the equal-key form; then medians over the steps."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.environ["GPUDRIVE_DEV"] = "1"
os.environ["GPUDRIVE_AMD_LIB"] = os.path.join(ROOT, "build", "expt", "expt_%s.so" % os.environ.get("EXPT", "clk"))
os.environ.setdefault("GPUDRIVE_MAX_AGENTS", "64")
sys.path.insert(0, ROOT)
import numpy as np, torch
import bench
wl = sys.argv[1] if len(sys.argv) > 1 else "synthetic"
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 40
W = 1024
dev = torch.device("cuda", 0)
sim = bench.make_sim(bench.scenes_for(wl, W, 0), bench.params_for(wl), 64, 0)
batches = bench.action_batches(W, 64, dev, seed=1234)
act = sim.action_tensor().to_torch()
TICK_US = 0.01
NAMES = ("setup", "fill", "make_heap", "rounds", "write_out")
rows = []
for k in range(steps):
    act.copy_(batches[k % 8]); sim.step()
    v = np.array([sim.stat(1000 + j) for j in range(234)], np.int64)
    waves = v[:224].reshape(32, 7).copy()
    ties_waves, ran, max_all, max_ties, max_free, blk_ties, blk_all, blk_chk, ins_chk, ins_redo = v[224:234]
    # per wave: blocks in the equal-key form, in the checked form, blocks
    w_blk_ties, w_blk_chk, w_blk_all = (waves[:, 5] >> 1) & 0x1ff, (waves[:, 5] >> 10) & 0x3ff, waves[:, 5] >> 20
    waves[:, 5] &= 1
    if ran == 0:
        continue
    slow = int(np.argmax(waves[:, 6]))
    ph = waves[slow, :5] * TICK_US
    first32_ties = int(waves[:, 5].sum())
    rows.append((*ph, waves[slow, 6] * TICK_US, max_all * TICK_US, max_ties * TICK_US, waves[slow, 5], ties_waves, ran, max_free * TICK_US,
                 100.0 * blk_ties / max(blk_all, 1), 100.0 * w_blk_ties[slow] / max(w_blk_all[slow], 1),
                 100.0 * blk_chk / max(blk_all, 1), 100.0 * ins_redo / max(ins_chk, 1)))
    if k >= 5:
        print("step %3d: slowest of first 32 = wave %2d%s: %s total %.1f | any wave %.1f, equal-key waves max %.1f | equal-key waves %d of %d (first 32: %d), %.1f %% of their blocks in the equal-key form (slowest of first 32: %d + %d checked of %d)" %
              (k + 1, slow, " (equal-key copy)" if waves[slow, 5] else "", " ".join("%s %.1f" % (n, x) for n, x in zip(NAMES, ph)),
               waves[slow, 6] * TICK_US, max_all * TICK_US, max_ties * TICK_US, ties_waves, ran, first32_ties, 100.0 * blk_ties / max(blk_all, 1), w_blk_ties[slow], w_blk_chk[slow], w_blk_all[slow]))
r = np.array(rows[5:], np.float64)
if len(r):
    med = np.median(r, axis=0)
    print("median over %d steps (us): %s total %.1f | any wave %.1f, equal-key max %.1f | slowest wave on the equal-key copy in %d of %d steps; "
          "last wave of the launch is an equal-key wave in %d of %d; equal-key waves %.0f of %.0f" %
          (len(r), " ".join("%s %.1f" % (n, x) for n, x in zip(NAMES, med[:5])), med[5], med[6], med[7], int(r[:, 8].sum()), len(r),
           int((r[:, 7] >= r[:, 6]).sum()), len(r), med[9], med[10]))
    print("slowest wave without equal keys: median %.1f us (min %.1f, max %.1f); the slowest equal-key wave lasts longer by a median of %.1f us" %
          (np.median(r[:, 11]), r[:, 11].min(), r[:, 11].max(), np.median(r[:, 7] - r[:, 11])))
    print("spread of the total (min .. max): %.1f .. %.1f; prologue (setup + fill + make_heap) median %.1f, min %.1f, max %.1f" %
          (r[:, 5].min(), r[:, 5].max(), np.median(r[:, :3].sum(1)), r[:, :3].sum(1).min(), r[:, :3].sum(1).max()))
    print("blocks in the equal-key form, of the blocks of the waves on the equal-key copy: median %.1f %% (min %.1f, max %.1f)" %
          (np.median(r[:, 12]), r[:, 12].min(), r[:, 12].max()))
    print("blocks in the checked form: median %.1f %% (min %.1f, max %.1f); inserts of its rounds redone in the equal-key form: median %.1f %% (min %.1f, max %.1f)" %
          (np.median(r[:, 14]), r[:, 14].min(), r[:, 14].max(), np.median(r[:, 15]), r[:, 15].min(), r[:, 15].max()))
sim.close()
