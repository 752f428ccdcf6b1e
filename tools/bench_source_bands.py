"""Time smi_stencil_run_source on a 2 x 2 LocalGroup (four rank threads on one GPU) of 4096^2
tiles, T = 90, at the library's default fusion setting.

usage: tools/bench_source_bands.py TREE SWITCH OUT
  TREE    a built checkout whose smi_amd package and library are timed ("." for this one; a
          checkout of the parent commit for the baseline -- one library per process)
  SWITCH  smi_stencil_set_source_bands (0 / 1); -1: leave it alone (a library without the switch)
  OUT     a .jsonl file the record is appended to

Per repetition: HIP events on each rank's stream around the run, the ranks released together by
a host barrier; the repetition's time is the slowest rank's.  6 warm-up runs, median of 15."""
import json
import statistics
import sys
import threading

tree, switch, out = sys.argv[1], int(sys.argv[2]), sys.argv[3]
sys.path.insert(0, tree)
import numpy as np
import torch
import smi_amd
from smi_amd import LocalGroup, stencil

X = Y = 4096
T, WARM, REPS = 90, 6, 15
smi_amd.load(build_if_missing=False)
torch.cuda.set_device(0)
if switch >= 0:
    stencil.set_source_bands(switch)
plan = stencil.plan(X, Y, 2, 2, 0, T, source=True)
bar = threading.Barrier(4)
rng = np.random.default_rng(1)
tiles = [rng.random((X, Y), dtype=np.float32) for _ in range(4)]
srcs = [rng.random((X, Y), dtype=np.float32) * np.float32(0.01) for _ in range(4)]


def rank_fn(comm):
    s = torch.cuda.Stream()
    times = []
    with torch.cuda.stream(s):
        t = torch.from_numpy(tiles[comm.rank]).cuda()
        src = torch.from_numpy(srcs[comm.rank]).cuda()
        scratch = torch.empty_like(t)
        for i in range(WARM + REPS):
            s.synchronize()
            bar.wait()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            stencil.run(comm, t, T, 2, 2, scratch=scratch, source=src)
            e1.record(s)
            s.synchronize()
            if i >= WARM:
                times.append(e0.elapsed_time(e1))
    return times


res = LocalGroup(4).run(rank_fn)
per_rep = [max(r[i] for r in res) for i in range(REPS)]
rec = {"tree": tree, "switch": switch, "plan": plan["phases"], "tile": [X, Y], "grid": [2, 2], "T": T,
       "reps": REPS, "median_ms": statistics.median(per_rep), "min_ms": min(per_rep), "max_ms": max(per_rep),
       "per_rep_ms": per_rep}
print(json.dumps(rec))
with open(out, "a") as f:
    f.write(json.dumps(rec) + "\n")
