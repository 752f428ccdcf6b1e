#!/usr/bin/env python3
"""What a convergence check costs (profiles/solve/).

Two measurements at 8192^2 on one GPU, appended as JSON lines to --out:

  --mode step   one library (--lib, default this tree's), loaded on its own
                with ctypes: smi_stencil_step timed over windows of --steps
                back-to-back single steps, --reps windows, device events
                around each window; if the library has it, the same for
                smi_stencil_step_residual, and for the unfused check a caller
                would otherwise write (a plain step plus a max|a - b| pass
                over both buffers).  Run it once per library -- the parent
                commit's and this tree's -- alternating, in fresh processes:
                two copies of the library in one process would share symbols.
  --mode solve  smi_stencil_solve against smi_stencil_run for the same number
                of steps (tol = 0 is never met on a random grid), check_every
                20, 100 and 400, host clock around the call and a stream
                synchronise; ms per step for both and the cost of one check
                (the single residual step, reduce, bcast, 4 bytes back and the
                host synchronise) = (solve - run) / checks.

  --mode fused  the fused check (smi_stencil_run_residual,
                smi_stencil_set_solve_check), everything alternating inside one
                process: (a) one K = 12 pass with and without the residual
                (sweepk_res_kernel<12> against sweepk_kernel<12>), device events
                around windows of --passes single-pass runs; (b)
                smi_stencil_run(T) against smi_stencil_run_residual(T) at T =
                20 and 100 under the default fusion, device events around
                windows of --runs runs; (c) solve against run as in --mode
                solve, with the solve check 0 and 1 alternating, so both
                per-check costs come from one session.

  --mode source the source term (smi_stencil_run_source) against the plain
                smi_stencil_run, alternating inside one process: one pass per
                call at steps_per_pass 1 and KS (smi_stencil_source_max_depth),
                device events around windows of --passes calls, every variant
                warmed with a full window first; ms per pass, and the ratio
                source / plain at the same depth (the source pass moves 12
                B/cell where the plain one moves 8 and runs without scaled
                levels).  Records go to profiles/source/ by default.

Not part of bench.py; a GPU is required.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def summary(ms: list[float]) -> dict:
    s = sorted(ms)
    return dict(median_ms=statistics.median(s), min_ms=s[0], max_ms=s[-1], stdev_ms=statistics.pstdev(s),
                p10_ms=s[len(s) // 10], p90_ms=s[-1 - len(s) // 10], reps=len(s))


def emit(out: str, rec: dict) -> None:
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    line = json.dumps(rec)
    print(line, flush=True)
    with open(out, "a") as f:
        f.write(line + "\n")


def mode_step(args) -> None:
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_solve needs a GPU")
    from smi_amd import build
    path = args.lib or build.lib_path()
    lib = ctypes.CDLL(path)      # torch's HIP runtime is loaded already
    P, I = ctypes.c_void_p, ctypes.c_int
    lib.smi_stencil_step.argtypes = [P, P, I, I, ctypes.POINTER(I), ctypes.POINTER(P), P, P, P]
    fused = getattr(lib, "smi_stencil_step_residual", None)
    if fused is not None:
        fused.argtypes = [P, P, I, I, ctypes.POINTER(I), ctypes.POINTER(P), P, P, P, P]
    N = args.size
    torch.manual_seed(0)
    a = torch.rand((N, N), device="cuda")
    b = torch.empty_like(a)
    word = torch.zeros(1, dtype=torch.int32, device="cuda")
    mode = (I * 4)(0, 0, 0, 0)
    halo = (P * 4)()
    stream = torch.cuda.current_stream().cuda_stream

    def plain(x, y):
        rc = lib.smi_stencil_step(x.data_ptr(), y.data_ptr(), N, N, mode, halo, None, None, stream)
        assert rc == 0, rc

    def with_residual(x, y):
        rc = fused(x.data_ptr(), y.data_ptr(), N, N, mode, halo, None, None, word.data_ptr(), stream)
        assert rc == 0, rc

    def unfused(x, y):
        plain(x, y)
        torch.max(torch.abs(y - x))     # what a caller writes without the fused step

    variants = [("plain_step", plain)]
    if fused is not None:
        variants.append(("fused_residual_step", with_residual))
    variants.append(("plain_step_plus_difference_pass", unfused))
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {name: [] for name, _ in variants}
    for name, fn in variants:           # warm every variant
        for _ in range(args.steps):
            fn(a, b)
            a, b = b, a
    torch.cuda.synchronize()
    for _ in range(args.reps):          # variants alternate inside every repetition
        for name, fn in variants:
            ev0.record()
            for _ in range(args.steps):
                fn(a, b)
                a, b = b, a
            ev1.record()
            ev1.synchronize()
            times[name].append(ev0.elapsed_time(ev1) / args.steps)
    for name, _ in variants:
        emit(args.out, dict(kind="step", label=args.label, variant=name, size=N, steps_per_window=args.steps,
                            unit="ms per step",
                            **summary(times[name])))


def mode_solve(args) -> None:
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_solve needs a GPU")
    import smi_amd
    from smi_amd import stencil
    N, T = args.size, args.total_steps
    comm = smi_amd.LocalGroup(1).comm(0)
    torch.manual_seed(0)
    src = torch.rand((N, N), device="cuda")
    tile, scratch = torch.empty_like(src), torch.empty_like(src)

    def run_once(fn) -> float:
        tile.copy_(src)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def do_run():
        stencil.run(comm, tile, T, 1, 1, scratch=scratch)

    for ce in (20, 100, 400):
        def do_solve():
            _, steps, r, conv = stencil.solve(comm, tile, 0.0, T, ce, 1, 1, scratch=scratch)
            assert steps == T and not conv, (steps, r, conv)

        for fn in (do_run, do_solve):
            run_once(fn)
        t_run, t_solve = [], []
        for _ in range(args.reps):      # alternating
            t_run.append(run_once(do_run))
            t_solve.append(run_once(do_solve))
        checks = (T + ce - 1) // ce
        run_s, solve_s = summary(t_run), summary(t_solve)
        emit(args.out, dict(kind="solve_vs_run", label=args.label, size=N, steps=T, check_every=ce, checks=checks,
                            run_ms_per_step=run_s["median_ms"] / T, solve_ms_per_step=solve_s["median_ms"] / T,
                            per_check_overhead_ms=(solve_s["median_ms"] - run_s["median_ms"]) / checks,
                            run_stdev_ms_per_step=run_s["stdev_ms"] / T, run=run_s, solve=solve_s))
    comm.finalize()


def mode_fused(args) -> None:
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_solve needs a GPU")
    import smi_amd
    from smi_amd import stencil
    N, T = args.size, args.total_steps
    comm = smi_amd.LocalGroup(1).comm(0)
    torch.manual_seed(0)
    src = torch.rand((N, N), device="cuda")
    tile, scratch = torch.empty_like(src), torch.empty_like(src)
    tile.copy_(src)
    word = torch.zeros(1, dtype=torch.int32, device="cuda")
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fuse0 = stencil.get_fusion()["steps_per_pass"]

    def window(fn, n) -> float:
        """ms per call over n back-to-back calls (device events); the buffers ping-pong"""
        a, b = tile, scratch
        ev0.record()
        for _ in range(n):
            res = fn(a, b)
            if res is b:
                a, b = b, a
        ev1.record()
        ev1.synchronize()
        return ev0.elapsed_time(ev1) / n

    def timed_pair(kind, steps, n, extra):
        def plain(a, b):
            return stencil.run(comm, a, steps, 1, 1, scratch=b)

        def resid(a, b):
            return stencil.run(comm, a, steps, 1, 1, scratch=b, residual=word)

        variants = [("run", plain), ("run_residual", resid)]
        times = {name: [] for name, _ in variants}
        for name, fn in variants:
            window(fn, n)
        for _ in range(args.reps):
            for name, fn in variants:
                times[name].append(window(fn, n))
        for name, _ in variants:
            emit(args.out, dict(kind=kind, label=args.label, variant=name, size=N, steps=steps, calls_per_window=n,
                                plan=stencil.plan(N, N, 1, 1, 0, steps, residual=name == "run_residual")["phases"],
                                unit="ms per call", **extra, **summary(times[name])))

    # (a) one K = 12 pass, residual instantiation against plain
    stencil.set_fusion(steps_per_pass=12)
    timed_pair("pass_k12", 12, args.passes, dict(steps_per_pass=12))
    # (b) whole runs under the default fusion
    stencil.set_fusion(steps_per_pass=fuse0)
    for steps in (20, 100):
        timed_pair("run_vs_run_residual", steps, args.runs, dict(steps_per_pass=fuse0))

    # (c) solve / run with both checks
    def run_once(fn) -> float:
        tile.copy_(src)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def do_run():
        stencil.run(comm, tile, T, 1, 1, scratch=scratch)

    check0 = stencil.get_solve_check()
    for ce in (20, 100, 400):
        def do_solve(fused):
            stencil.set_solve_check(fused)
            _, steps, r, conv = stencil.solve(comm, tile, 0.0, T, ce, 1, 1, scratch=scratch)
            assert steps == T and not conv, (steps, r, conv)

        fns = [("run", do_run), ("solve_check0", lambda: do_solve(0)), ("solve_check1", lambda: do_solve(1))]
        for _, fn in fns:
            run_once(fn)
        t = {name: [] for name, _ in fns}
        for _ in range(args.reps):      # alternating
            for name, fn in fns:
                t[name].append(run_once(fn))
        checks = (T + ce - 1) // ce
        sm = {name: summary(v) for name, v in t.items()}
        per_check = {name: [(s - r) / checks for s, r in zip(t[name], t["run"])] for name in ("solve_check0",
                                                                                              "solve_check1")}
        emit(args.out, dict(kind="solve_vs_run_checks", label=args.label, size=N, steps=T, check_every=ce,
                            checks=checks, run_ms_per_step=sm["run"]["median_ms"] / T,
                            solve0_ms_per_step=sm["solve_check0"]["median_ms"] / T,
                            solve1_ms_per_step=sm["solve_check1"]["median_ms"] / T,
                            per_check_ms_check0=summary(per_check["solve_check0"]),
                            per_check_ms_check1=summary(per_check["solve_check1"]),
                            run=sm["run"], solve_check0=sm["solve_check0"], solve_check1=sm["solve_check1"]))
    stencil.set_solve_check(check0)
    comm.finalize()


def mode_source(args) -> None:
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_solve needs a GPU")
    import smi_amd
    from smi_amd import stencil
    N = args.size
    comm = smi_amd.LocalGroup(1).comm(0)
    torch.manual_seed(0)
    tile = torch.rand((N, N), device="cuda")
    scratch = torch.empty_like(tile)
    g = torch.rand((N, N), device="cuda") * 1e-3
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fuse0 = stencil.get_fusion()["steps_per_pass"]
    KS = stencil.source_max_depth()

    def window(fn, n) -> float:
        a, b = tile, scratch
        ev0.record()
        for _ in range(n):
            res = fn(a, b)
            if res is b:
                a, b = b, a
        ev1.record()
        ev1.synchronize()
        return ev0.elapsed_time(ev1) / n

    for K in (1, KS):
        stencil.set_fusion(steps_per_pass=K, rows_per_wave=-1 if K >= 3 else 0)
        assert stencil.plan(N, N, 1, 1, 0, K, source=True)["phases"] == [(K, 1)]
        assert stencil.plan(N, N, 1, 1, 0, K)["phases"] == [(K, 1)]
        variants = [("run", lambda a, b: stencil.run(comm, a, K, 1, 1, scratch=b)),
                    ("run_source", lambda a, b: stencil.run(comm, a, K, 1, 1, scratch=b, source=g))]
        times = {name: [] for name, _ in variants}
        for _, fn in variants:          # warm every variant at the timed shape
            window(fn, args.passes)
        for _ in range(args.reps):      # alternating
            for name, fn in variants:
                times[name].append(window(fn, args.passes))
        sm = {name: summary(v) for name, v in times.items()}
        for name, _ in variants:
            emit(args.out, dict(kind="source_pass", label=args.label, variant=name, size=N, steps_per_pass=K,
                                calls_per_window=args.passes, unit="ms per pass", **sm[name]))
        emit(args.out, dict(kind="source_vs_plain", label=args.label, size=N, steps_per_pass=K,
                            ratio_of_medians=sm["run_source"]["median_ms"] / sm["run"]["median_ms"],
                            bytes_per_cell=dict(run=8, run_source=12)))
    stencil.set_fusion(steps_per_pass=fuse0)
    comm.finalize()


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mode", choices=("step", "solve", "fused", "source"), required=True)
    ap.add_argument("--lib", default=None, help="step mode: the libsmi_amd.so to time (default: this tree's)")
    ap.add_argument("--label", default="current", help="recorded with every line (e.g. parent / current)")
    ap.add_argument("--size", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--steps", type=int, default=200, help="step mode: single steps per timed window")
    ap.add_argument("--total-steps", type=int, default=2000, help="solve mode: steps of every run / solve")
    ap.add_argument("--passes", type=int, default=100, help="fused mode: K = 12 passes per timed window")
    ap.add_argument("--runs", type=int, default=20, help="fused mode: runs per timed window")
    ap.add_argument("--out", default=None, help="default: profiles/solve/solve.jsonl (source mode: "
                                                "profiles/source/source.jsonl)")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", *(("source", "source.jsonl") if args.mode == "source"
                                                    else ("solve", "solve.jsonl")))
    {"step": mode_step, "solve": mode_solve, "fused": mode_fused, "source": mode_source}[args.mode](args)


if __name__ == "__main__":
    main()
