#!/usr/bin/env python3
"""One rank of the multi-process smi_allreduce run (started by
tests/test_allreduce_rccl_gpu.py as a fresh child process, never exec'd).

Production path: gloo process group for the control plane, the RCCL unique id
through its store, smi_init (Comm.from_env).  Cases, each bit for bit against
the CPU oracle on every rank: smi_allreduce below, at and above the 256 KiB
switch, pipelined in several pieces and in place (fp32 add, int32 max, double
add); smi_kmeans under set_means(1); one smi_stencil_solve, whose check points
go through the integer-max allreduce.

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
from smi_amd import collectives, kmeans, stencil  # noqa: E402

OK = True
FLOAT, INT, DOUBLE = 2, 1, 3
ADD, MAX = 0, 1
TOL, CHECK_EVERY, MAX_STEPS = 1e-3, 20, 600
XL, YL = 32, 64


def report(rank, name, good):
    global OK
    OK &= bool(good)
    print(f"[{rank}] CASE {name} {'OK' if good else 'MISMATCH'}", flush=True)


def contribs(n, count, t, seed):
    rng = np.random.default_rng(seed)
    npdt = oracle.NP_DTYPE[t]
    if t in (FLOAT, DOUBLE):
        return (rng.random((n, count)) * 2 - 1).astype(npdt) * npdt(1000.0)
    info = np.iinfo(npdt)
    return rng.integers(info.min, info.max, size=(n, count), endpoint=True, dtype=npdt)


def allreduce_cases(comm, rank, world, s):
    old = collectives.get_pipeline_bytes()
    try:
        # (name, count, piece bytes, in place): fp32 counts around 65536 = 256 KiB
        for name, count, pb, in_place in (("small", 300, old, False), ("boundary", 65536, old, False),
                                          ("past boundary", 65537, old, False),
                                          ("pipelined", 70001, 16384, False), ("in place small", 300, old, True),
                                          ("in place pipelined", 70001, 16384, True)):
            collectives.set_pipeline_bytes(pb)
            for t, op, tag in ((FLOAT, ADD, "fp32 add"), (INT, MAX, "int32 max"), (DOUBLE, ADD, "double add")):
                c = contribs(world, count, t, seed=count + t)
                snd = torch.from_numpy(c[rank].copy()).cuda()
                rcv = None if in_place else torch.zeros_like(snd)
                got = collectives.allreduce(comm, snd, rcv, op)
                s.synchronize()
                want = oracle.reduce(c, t, op)
                report(rank, f"allreduce {name} {tag}", np.array_equal(got.cpu().numpy().view(np.uint8),
                                                                       want.view(np.uint8)))
    finally:
        collectives.set_pipeline_bytes(old)


def same_bits(a, b):
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


def kmeans_case(comm, rank, world, s):
    rng = np.random.default_rng(17)
    clusters, dims, iters = 8, 64, 3
    n = 64 * world
    centres = rng.random((clusters, dims), dtype=np.float32) * 10 - 5
    pts = rng.standard_normal((n, dims), dtype=np.float32) + centres[np.arange(n) % clusters]
    cen0 = pts[:clusters].copy()
    want = oracle.kmeans(pts, cen0, iters, ranks=world, width=16)
    kmeans.set_means(1)
    try:
        c = torch.from_numpy(cen0.copy()).cuda()
        local = torch.from_numpy(np.ascontiguousarray(kmeans.split_points(pts, world, rank))).cuda()
        kmeans.kmeans(comm, local, c, iters, width=16)
        s.synchronize()
    finally:
        kmeans.set_means(0)
    report(rank, "kmeans means mode 1", same_bits(c.cpu().numpy(), want))


def resid(new, old):
    with np.errstate(invalid="ignore"):
        d = np.abs(new - old)
    return np.float32(np.nan) if np.isnan(d).any() else np.float32(d.max())


def expected_solve(g):
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


def solve_case(comm, rank, world, s):
    PX, PY = 1, world
    g = stencil.init_grid(XL * PX, YL * PY)
    tiles = stencil.split_memory(g, PX, PY)
    t = torch.from_numpy(tiles[rank]).cuda()
    res, steps, r, conv = stencil.solve(comm, t, TOL, MAX_STEPS, CHECK_EVERY, PX, PY)
    s.synchronize()
    out = [None] * world
    dist.all_gather_object(out, (res.cpu().numpy(), steps, int(np.float32(r).view(np.uint32)), conv))
    steps_w, r_w, x_w = expected_solve(g)
    name = f"solve {PX}x{PY}"
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
            allreduce_cases(comm, rank, world, s)
            kmeans_case(comm, rank, world, s)
            solve_case(comm, rank, world, s)
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
        print("ALLREDUCE MULTIPROC", "PASS" if flag.item() else "FAIL", flush=True)
    sys.exit(0 if flag.item() else 1)


if __name__ == "__main__":
    main()
