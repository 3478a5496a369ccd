#!/usr/bin/env python3
"""developer tool: when the waves of k_knn_rank's standard launch end (tools/build_expt.sh wclk -DGD_WAVE_CLOCKS: the product's
code plus three stores per wave; engine.hpp GD_RH_WAVES: per wave the 100 MHz clock at its start and end, the agents it ranked).
  EXPT=wclk python3 tools/rank_waves.py [synthetic|waymo|cfg3] [samples]
Per sample (the last of 30 steps run back to back) and as medians over the samples, for the whole launch and per XCD
(workgroup b runs on XCD b % 8): mean, median and maximum end of the waves that ranked an agent, measured from the earliest
start of the launch on the wave's XCD (us); the share of the waves' time that lies after the median end (sum of end - median
over the later half / sum of the ends); how long the slowest wave ends after the mean one; the busy share (sum of end - start
over all waves / resident waves x last end, 16 waves per CU resident); agents per wave (min / mean / max)."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.environ["GPUDRIVE_DEV"] = "1"
os.environ["GPUDRIVE_AMD_LIB"] = os.path.join(ROOT, "build", "expt", "expt_%s.so" % os.environ.get("EXPT", "wclk"))
os.environ.setdefault("GPUDRIVE_MAX_AGENTS", "64")
sys.path.insert(0, ROOT)
import numpy as np, torch
import bench
wl = sys.argv[1] if len(sys.argv) > 1 else "synthetic"
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 8  # samples
BURST = 30
W = 1024
GRID = 256 * 8 * 4  # engine.hpp GD_RANK_GRID
dev = torch.device("cuda", 0)
sim = bench.make_sim(bench.scenes_for(wl, W, 0), bench.params_for(wl), 64, 0)
batches = bench.action_batches(W, 64, dev, seed=1234)
act = sim.action_tensor().to_torch()
nw = int(os.environ.get("GPUDRIVE_RANK_WAVES", "0")) or min((sim.stat(5) + 7) // 8 * 8, GRID)
resident = min(nw, 256 * 16)
TICK_US = 0.01


def figures(start, end, turns, slots):
    on = turns > 0
    e = end[on].astype(np.int32) * TICK_US
    med = float(np.median(e))
    busy = ((end - start).astype(np.int32)).sum() * TICK_US / (slots * e.max())
    return (e.mean(), med, e.max(), 100.0 * np.maximum(e - med, 0.0).sum() / e.sum(), 100.0 * (e.max() / e.mean() - 1.0), 100.0 * busy,
            turns[on].min(), turns[on].mean(), turns.max())


FMT = "mean %6.1f median %6.1f max %6.1f us | after the median %4.1f %% | slowest / mean +%4.1f %% | busy %4.1f %% | agents per wave %d / %.1f / %d"
rows = []
done = 0
for k in range(steps):
    # a burst of steps back to back, the clocks of its last one: reading them takes the host half a second, and a launch
    # behind such a pause runs on a chip that has clocked down (seen: 900 us for a kernel of 400)
    for j in range(BURST):
        if done and done % 91 == 0:
            sim.reset(list(range(W)))  # (bench.py: a reset of all worlds every 91 steps, the episode length)
        act.copy_(batches[done % 8]); sim.step()
        done += 1
    v = np.array([sim.stat(2000 + j * GRID + b) for j in range(3) for b in range(nw)], np.int64).reshape(3, nw)
    start, end, turns = v[0].astype(np.uint32), v[1].astype(np.uint32), v[2]
    # every XCD counts from its own earliest start: the XCDs' clocks are not aligned with each other (seen: the same launch
    # "ended" between 498 and 950 us after the chip's earliest start, depending on the XCD).  Low 32 bits: differences wrap correctly
    for x in range(8):
        t0 = start[x::8][int((start[x::8] - start[x]).astype(np.int32).argmin())]
        start[x::8] -= t0
        end[x::8] -= t0
    row = [figures(start, end, turns, resident)] + [figures(start[x::8], end[x::8], turns[x::8], resident / 8) for x in range(8)]
    rows.append(row)
    print("step %3d: %s" % (k + 1, FMT % row[0]))
r = np.median(np.array(rows, np.float64), axis=0)
print("medians over %d samples, %d waves, %d resident" % (len(rows), nw, resident))
print("  all  : " + FMT % tuple(r[0]))
for x in range(8):
    print("  XCD %d: " % x + FMT % tuple(r[1 + x]))
sim.close()
