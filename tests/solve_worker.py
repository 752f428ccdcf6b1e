#!/usr/bin/env python3
"""One rank of the two-process smi_stencil_solve run (started by
tests/test_stencil_solve_gpu.py as a fresh child process, never exec'd).

Production path: gloo process group for the control plane, the RCCL unique id
through its store, smi_init (Comm.from_env), then smi_stencil_solve on the
1x2 and the 2x1 decomposition of 32x64 tiles -- halo exchanges, the integer-max
reduce and the bcast of the residual word all on the one RCCL communicator.
Steps, residual bits and the combined grid are checked bit for bit against the
CPU oracle, and every rank must report the same steps and residual.

Prints "CASE <name> OK|MISMATCH" lines and exits 0 only if every rank passed.
"""
import os
import sys
import traceback

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

import oracle  # noqa: E402
import smi_amd  # noqa: E402
from smi_amd import stencil  # noqa: E402

OK = True
TOL, CHECK_EVERY, MAX_STEPS = 1e-3, 20, 600
XL, YL = 32, 64


def report(rank, name, good):
    global OK
    OK &= bool(good)
    print(f"[{rank}] CASE {name} {'OK' if good else 'MISMATCH'}", flush=True)


def resid(new, old):
    with np.errstate(invalid="ignore"):
        d = np.abs(new - old)
    return np.float32(np.nan) if np.isnan(d).any() else np.float32(d.max())


def expected(g):
    """(steps, residual, state) at the first check point with r_t <= TOL."""
    x, t, r = g, 0, np.float32(np.inf)
    while t < MAX_STEPS:
        nxt = min(t + CHECK_EVERY, MAX_STEPS)
        prev = oracle.stencil(x, nxt - t - 1)
        x = oracle.stencil(prev, 1)
        r, t = resid(x, prev), nxt
        if r <= np.float32(TOL):
            break
    return t, r, x


def solve_cases(comm, rank, world, s):
    for PX, PY in ((1, 2), (2, 1)):
        g = stencil.init_grid(XL * PX, YL * PY)
        tiles = stencil.split_memory(g, PX, PY)
        t = torch.from_numpy(tiles[rank]).cuda()
        res, steps, r, conv = stencil.solve(comm, t, TOL, MAX_STEPS, CHECK_EVERY, PX, PY)
        s.synchronize()
        out = [None] * world
        dist.all_gather_object(out, (res.cpu().numpy(), steps, int(np.float32(r).view(np.uint32)), conv))
        if rank == 0:
            steps_w, r_w, x_w = expected(g)
            name = f"solve {PX}x{PY}"
            print(f"[0] {name}: steps {[o[1] for o in out]} want {steps_w}, residual {r} want {r_w}", flush=True)
            report(rank, f"{name} steps", all(o[1] == steps_w for o in out))
            report(rank, f"{name} residual bits", all(o[2] == int(r_w.view(np.uint32)) for o in out))
            report(rank, f"{name} converged", all(o[3] == bool(r_w <= np.float32(TOL)) for o in out))
            got = stencil.combine_memory([o[0] for o in out], PX, PY)
            report(rank, f"{name} grid", np.array_equal(got.view(np.uint32), x_w.view(np.uint32)))


def main():
    rank = int(os.environ["RANK"])
    world = int(os.environ["WORLD_SIZE"])
    dev = int(os.environ.get("LOCAL_RANK", "0")) % max(1, torch.cuda.device_count())
    torch.cuda.set_device(dev)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    comm = smi_amd.Comm.from_env(device=dev)
    s = torch.cuda.Stream()
    global OK
    try:
        with torch.cuda.stream(s):
            solve_cases(comm, rank, world, s)
            s.synchronize()
            dist.barrier()
    except Exception:  # noqa: BLE001
        traceback.print_exc()
        OK = False
    comm.finalize()
    flag = torch.tensor([1 if OK else 0])
    dist.all_reduce(flag, op=dist.ReduceOp.MIN)
    dist.destroy_process_group()
    if rank == 0:
        print("SOLVE MULTIPROC", "PASS" if flag.item() else "FAIL", flush=True)
    sys.exit(0 if flag.item() else 1)


if __name__ == "__main__":
    main()
