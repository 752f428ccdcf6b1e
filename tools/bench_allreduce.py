#!/usr/bin/env python3
"""smi_allreduce against smi_reduce followed by smi_bcast, and smi_kmeans with
set_means 0 against 1.

  --mode local   N rank threads on one GPU (LocalGroup; device copies stand in
                 for the links)
  --mode rccl    N fresh child processes, one rank each, over RCCL (sockets on
                 a one-GPU box); the parent starts them with subprocess and
                 never touches the GPU
  --mode kmeans  per-iteration time of smi_kmeans at the reference shape
                 (8 clusters x 64 dims, W = 16), N rank threads, mode 0 and 1

One call = one collective (or the pair) on the rank's stream; a sample is the
HIP-event time of `--calls` back-to-back calls divided by their number, taken
after `--warmup` untimed samples; the two sides alternate sample by sample.
Per size the line carries the median and the p10/p90 of the slowest rank's
samples.  One JSON line per size on stdout.
"""
import argparse
import json
import os
import socket
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = [4, 2048, 256 << 10, (256 << 10) + 4, 1 << 20, 64 << 20]  # bytes of fp32


def _samples(comm, nbytes, calls, warmup, reps, sync):
    import torch
    from smi_amd import collectives
    count = nbytes // 4
    s = torch.cuda.Stream()
    out = {"allreduce": [], "reduce_bcast": []}
    with torch.cuda.stream(s):
        snd = torch.full((count,), float(comm.rank + 1), device="cuda")
        rcv = torch.zeros_like(snd)

        def allreduce():
            collectives.allreduce(comm, snd, rcv, "add")

        def pair():
            collectives.reduce(comm, snd, rcv, "add", root=0)
            collectives.bcast(comm, rcv, root=0)

        for i in range(warmup + reps):
            for name, fn in (("allreduce", allreduce), ("reduce_bcast", pair)):
                sync()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(s)
                for _ in range(calls):
                    fn()
                b.record(s)
                s.synchronize()
                if i >= warmup:
                    out[name].append(a.elapsed_time(b) * 1e3 / calls)  # us per call
    return out


def _line(tag, nbytes, per_rank):
    import numpy as np
    rec = {"bench": tag, "bytes": nbytes}
    for name in per_rank[0]:
        worst = np.max(np.array([r[name] for r in per_rank]), axis=0)  # a sample = its slowest rank
        rec[name + "_us"] = {"median": round(float(np.median(worst)), 2),
                             "p10": round(float(np.percentile(worst, 10)), 2),
                             "p90": round(float(np.percentile(worst, 90)), 2)}
    print(json.dumps(rec), flush=True)


def _calls(nbytes, calls):
    return max(2, calls // 8) if nbytes >= (1 << 20) else calls


def run_local(args):
    import threading
    import smi_amd
    bar = threading.Barrier(args.ranks)
    for nbytes in SIZES:
        if nbytes > args.max_bytes:
            continue
        res = smi_amd.LocalGroup(args.ranks).run(
            lambda comm: _samples(comm, nbytes, _calls(nbytes, args.calls), args.warmup, args.reps, bar.wait))
        _line(f"local{args.ranks}", nbytes, res)


def run_rccl_child(args):
    import torch
    import torch.distributed as dist
    import smi_amd
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dev = int(os.environ.get("LOCAL_RANK", "0")) % max(1, torch.cuda.device_count())
    torch.cuda.set_device(dev)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    comm = smi_amd.Comm.from_env(device=dev)
    for nbytes in SIZES:
        if nbytes > args.max_bytes:
            continue
        mine = _samples(comm, nbytes, _calls(nbytes, args.calls), args.warmup, args.reps, dist.barrier)
        allr = [None] * world
        dist.all_gather_object(allr, mine)
        if rank == 0:
            _line(f"rccl{world}", nbytes, allr)
    comm.finalize()
    dist.destroy_process_group()


def run_rccl_parent(args):
    import torch
    ngpu = torch.cuda.device_count()  # does not initialise the GPU
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    procs = []
    for r in range(args.ranks):
        env = dict(os.environ)
        env.update(RANK=str(r), WORLD_SIZE=str(args.ranks), LOCAL_RANK=str(r % max(1, ngpu)),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
        if ngpu < args.ranks:
            env.update(NCCL_HOSTID=f"smi-bench-host-{r}", NCCL_SOCKET_IFNAME="lo", NCCL_IB_DISABLE="1")
        cmd = [sys.executable, "-u", os.path.abspath(__file__), "--mode", "rccl-child", "--calls", str(args.calls),
               "--warmup", str(args.warmup), "--reps", str(args.reps), "--max-bytes", str(args.max_bytes)]
        procs.append(subprocess.Popen(cmd, env=env))
    rc = 0
    for p in procs:
        try:
            rc |= p.wait(timeout=args.limit)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            rc = 1
    sys.exit(rc)


def run_kmeans(args):
    import threading
    import numpy as np
    import torch
    import smi_amd
    from smi_amd import kmeans
    bar = threading.Barrier(args.ranks)
    iters = 20
    pts, cen0 = kmeans.synthetic_points(args.points * args.ranks, seed=5)
    pts, cen0 = pts.numpy(), cen0.numpy()

    def fn(comm):
        s = torch.cuda.Stream()
        out = []
        with torch.cuda.stream(s):
            local = torch.from_numpy(np.ascontiguousarray(kmeans.split_points(pts, comm.size, comm.rank))).cuda()
            for i in range(args.warmup + args.reps):
                c = torch.from_numpy(cen0.copy()).cuda()
                bar.wait()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(s)
                kmeans.kmeans(comm, local, c, iters)
                b.record(s)
                s.synchronize()
                if i >= args.warmup:
                    out.append(a.elapsed_time(b) * 1e3 / iters)
        return out

    rec = {"bench": f"kmeans local{args.ranks}", "points_per_rank": args.points, "iterations": iters}
    for mode in (0, 1, 0, 1):
        kmeans.set_means(mode)
        try:
            res = smi_amd.LocalGroup(args.ranks).run(fn)
        finally:
            kmeans.set_means(0)
        worst = np.max(np.array(res), axis=0)
        rec.setdefault(f"mode{mode}_us_per_iteration", []).append(
            {"median": round(float(np.median(worst)), 2), "p10": round(float(np.percentile(worst, 10)), 2),
             "p90": round(float(np.percentile(worst, 90)), 2)})
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["local", "rccl", "rccl-child", "kmeans"], default="local")
    ap.add_argument("--ranks", type=int, default=8)
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--points", type=int, default=4096)
    ap.add_argument("--max-bytes", type=int, default=64 << 20)
    ap.add_argument("--limit", type=int, default=500)
    a = ap.parse_args()
    {"local": run_local, "rccl": run_rccl_parent, "rccl-child": run_rccl_child, "kmeans": run_kmeans}[a.mode](a)
