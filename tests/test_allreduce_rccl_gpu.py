"""smi_allreduce on the production RCCL transport: 2 and 4 fresh child
processes (tests/allreduce_worker.py), one rank each, through smi_init --
small, boundary, pipelined and in-place allreduces, smi_kmeans under
set_means(1) and one smi_stencil_solve, every case bit-exact vs the oracle.

On a one-GPU box every child gets its own NCCL_HOSTID in its environment
before it starts (RCCL refuses two ranks on one device of one host), so the
bytes move over RCCL's socket transport.  The parent never touches the GPU
itself and never execs: the children are started with subprocess and killed
if they outlive the time limit.
"""
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _launch(world, timeout=240):
    import torch
    ngpu = torch.cuda.device_count()  # does not initialise the GPU on this image
    port = _free_port()
    procs = []
    for r in range(world):
        env = dict(os.environ)
        env.update(RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK=str(r % max(1, ngpu)),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
        if ngpu < world:
            env.update(NCCL_HOSTID=f"smi-test-host-{r}", NCCL_SOCKET_IFNAME="lo", NCCL_IB_DISABLE="1")
        procs.append(subprocess.Popen([sys.executable, "-u", os.path.join(HERE, "allreduce_worker.py")], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs, rcs = [], []
    for p in procs:
        try:
            out, _ = p.communicate(timeout=timeout)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            out, _ = p.communicate()
            out += "\n<killed: time limit>"
        outs.append(out)
        rcs.append(p.returncode)
    return rcs, outs


@pytest.mark.parametrize("world", [2, 4])
def test_allreduce_rccl_multiprocess(world):
    import torch
    if torch.cuda.device_count() == 0:  # counts devices without initialising the GPU
        pytest.skip("no GPU visible")
    rcs, outs = _launch(world)
    log = "\n".join(f"--- rank {r} (rc {rc})\n{o[-4000:]}" for r, (rc, o) in enumerate(zip(rcs, outs)))
    print(log)
    assert all(rc == 0 for rc in rcs), log
    assert "ALLREDUCE MULTIPROC PASS" in outs[0], log
    # per rank: 6 x 3 allreduce cases, kmeans, 4 solve checks
    for o in outs:
        assert o.count(" CASE ") == 23 and "MISMATCH" not in o, log
