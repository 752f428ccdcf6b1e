#!/usr/bin/env python3
"""One rank of the two-process smi_stencil_solve run with the fused check
(started by tests/test_stencil_run_residual_gpu.py as a fresh child process,
never exec'd): tests/solve_worker.py's cases and checks, unchanged, after
smi_stencil_set_solve_check(1) -- so every check point's residual comes out of
a K-step residual pass (band kernel + interior sweep over the RCCL exchange)
instead of a single step."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import solve_worker  # noqa: E402  (puts the repository root on sys.path)
from smi_amd import stencil  # noqa: E402

if __name__ == "__main__":
    stencil.set_solve_check(1)
    print("SOLVE CHECK FUSED", stencil.get_solve_check(), flush=True)
    solve_worker.main()
