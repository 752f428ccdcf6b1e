"""smi_allreduce on the GPU: on every rank the bytes smi_reduce leaves on its
root -- the oracle's canonical rank-order fold (codegen/templates/reduce.cl:
42-148) -- on both schedules (one all-to-all round and one fold up to 256 KiB,
the owner-chunk pipeline with an all-gather above), in place and out of
place.  Multi-rank cases run as an in-process rank group on one GPU.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FLOAT, INT, DOUBLE, CHAR = 2, 1, 3, 4
ADD, MAX, MIN = 0, 1, 2


def _contribs(oracle_mod, n, count, t, seed):
    rng = np.random.default_rng(seed)
    npdt = oracle_mod.NP_DTYPE[t]
    if t in (2, 3):
        return (rng.random((n, count)) * 2 - 1).astype(npdt) * npdt(1000.0)
    info = np.iinfo(npdt)
    return rng.integers(info.min, info.max, size=(n, count), endpoint=True, dtype=npdt)


def _group_allreduce(n, cases, in_place=False):
    """cases: a list of ((n, count) contributions, op).  Every rank runs them
    in order on one communicator and one stream; returns, per rank, the list
    of result arrays."""
    from smi_amd import LocalGroup, collectives

    def fn(comm):
        s = torch.cuda.Stream()
        outs = []
        with torch.cuda.stream(s):
            for c, op in cases:
                snd = torch.from_numpy(np.ascontiguousarray(c[comm.rank])).cuda()
                if in_place:
                    got = collectives.allreduce(comm, snd, None, op)
                    assert got is snd
                else:
                    keep = snd.clone()
                    got = torch.zeros_like(snd)
                    collectives.allreduce(comm, snd, got, op)
                    outs.append(("send", snd, keep))
                outs.append(("recv", got, None))
            s.synchronize()
        res = []
        for kind, a, b in outs:
            if kind == "send":  # the send buffer of an out-of-place call is left alone
                assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
            else:
                res.append(a.cpu().numpy())
        return res

    return LocalGroup(n).run(fn)


def _check(oracle_mod, n, cases, t, in_place=False):
    per_rank = _group_allreduce(n, cases, in_place)
    for i, (c, op) in enumerate(cases):
        want = oracle_mod.reduce(np.ascontiguousarray(c), t, op).view(np.uint8)
        for r in range(n):
            assert np.array_equal(per_rank[r][i].view(np.uint8), want), (n, t, op, c.shape[1], r)


@pytest.mark.parametrize("t", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("op", [0, 1, 2])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 8])
def test_allreduce_matches_oracle_on_every_rank(gpu, oracle_mod, t, op, n):
    cases = [(_contribs(oracle_mod, n, count, t, seed=count * 11 + n + op), op) for count in (1, 7, 300, 4099)]
    _check(oracle_mod, n, cases, t)


@pytest.mark.parametrize("n", [2, 8])
def test_allreduce_special_values(gpu, oracle_mod, n):
    """-0.0 on every rank adds up to +0.0 (the +0 start); a NaN on one rank
    propagates; an all-negative column under MAX gives FLT_MIN, the start value
    the reference has; the bytes are the same on every rank."""
    c = np.zeros((n, 8), np.float32)
    c[:, 0] = -0.0
    c[:, 1] = 1.0
    c[n - 1, 1] = np.nan
    c[:, 2] = -np.arange(1, n + 1)
    c[:, 3] = np.arange(n) - 0.5
    c[0, 4] = np.nan
    c[:, 5] = -0.0
    c[n // 2, 5] = 0.0
    c[:, 6] = np.inf
    c[n - 1, 6] = -np.inf
    c[:, 7] = 1e-40  # subnormal
    cases = [(c, op) for op in (ADD, MAX, MIN)]
    per_rank = _group_allreduce(n, cases)
    for i, (_, op) in enumerate(cases):
        want = oracle_mod.reduce(c, FLOAT, op)
        for r in range(n):
            assert np.array_equal(per_rank[r][i].view(np.uint32), want.view(np.uint32)), (op, r)
            assert np.array_equal(per_rank[r][i].view(np.uint32), per_rank[0][i].view(np.uint32))
    add, mx = per_rank[0][0], per_rank[0][1]
    assert add.view(np.uint32)[0] == 0  # +0.0, not -0.0
    assert np.isnan(add[1]) and np.isnan(add[4]) and np.isnan(add[6])
    assert mx[2] == np.finfo(np.float32).tiny


@pytest.fixture
def piece_bytes():
    """Set the pipeline piece size for one test, restore after."""
    from smi_amd import collectives
    old = collectives.get_pipeline_bytes()
    try:
        yield collectives.set_pipeline_bytes
    finally:
        collectives.set_pipeline_bytes(old)


@pytest.mark.parametrize("n", [3, 8])
def test_allreduce_path_boundary(gpu, oracle_mod, n):
    """fp32 count 65536 is exactly 256 KiB (one round, one fold); 65537 takes
    the owner-chunk pipeline."""
    cases = [(_contribs(oracle_mod, n, count, FLOAT, seed=count + n), ADD) for count in (65536, 65537)]
    _check(oracle_mod, n, cases, FLOAT)


@pytest.mark.parametrize("pb", [16384, 0])
def test_allreduce_pipelined_pieces(gpu, oracle_mod, piece_bytes, pb):
    """70001 fp32 on 3 ranks: chunks of 23336 elements (the last one 23329);
    16 KiB pieces cut a chunk into 6 pieces of 3892, the last one shorter, and
    the short chunk's last piece shorter still.  0: one piece per chunk."""
    piece_bytes(pb)
    n, count = 3, 70001
    cases = [(_contribs(oracle_mod, n, count, FLOAT, seed=pb + op), op) for op in (ADD, MAX)]
    _check(oracle_mod, n, cases, FLOAT)


def test_allreduce_pipelined_int8_eight_ranks(gpu, oracle_mod):
    """262145 one-byte elements: one past the switch, 16-element chunk rounding."""
    n, count = 8, 262145
    _check(oracle_mod, n, [(_contribs(oracle_mod, n, count, CHAR, seed=8), ADD)], CHAR)


@pytest.mark.parametrize("count", [300, 70001])
def test_allreduce_in_place(gpu, oracle_mod, piece_bytes, count):
    """send is recv, on the small path and on the pipeline (several pieces)."""
    piece_bytes(16384)
    n = 4
    cases = [(_contribs(oracle_mod, n, count, t, seed=count + t), ADD) for t in (FLOAT,)]
    _check(oracle_mod, n, cases, FLOAT, in_place=True)
    cases = [(_contribs(oracle_mod, n, count, DOUBLE, seed=count), MIN)]
    _check(oracle_mod, n, cases, DOUBLE, in_place=True)


def test_allreduce_partial_overlap_refused(gpu):
    """recv overlapping send anywhere but at send itself: an argument error on
    every rank, before any device call -- nothing is written."""
    from smi_amd import LocalGroup, SMIError, collectives

    def fn(comm):
        buf = torch.arange(600, dtype=torch.float32, device="cuda")
        keep = buf.clone()
        for lo in (100, 299):      # recv starts inside send
            with pytest.raises(SMIError, match="overlap"):
                collectives.allreduce(comm, buf[:300], buf[lo:lo + 300], "add")
        with pytest.raises(SMIError, match="overlap"):  # send starts inside recv
            collectives.allreduce(comm, buf[200:500], buf[:300], "add")
        torch.cuda.synchronize()
        assert torch.equal(buf, keep)
        # adjacent ranges do not overlap
        collectives.allreduce(comm, buf[:300], buf[300:], "add")
        torch.cuda.synchronize()
        return buf.cpu().numpy()

    for got in LocalGroup(2).run(fn):
        assert np.array_equal(got[:300], np.arange(300, dtype=np.float32))
        assert np.array_equal(got[300:], 2 * np.arange(300, dtype=np.float32))


def test_allreduce_reduce_bcast_allreduce_on_one_stream(gpu, oracle_mod):
    """A sequence on one communicator and one stream with no host
    synchronisation in between: the workspace the allreduce's fold reads is
    the one the reduce's root stages into next."""
    from smi_amd import LocalGroup, collectives
    n = 4
    a = _contribs(oracle_mod, n, 5000, FLOAT, seed=1)
    b = _contribs(oracle_mod, n, 6000, INT, seed=2)
    d = _contribs(oracle_mod, n, 4099, DOUBLE, seed=3)

    def fn(comm):
        s = torch.cuda.Stream()
        r = comm.rank
        with torch.cuda.stream(s):
            ta, tb, td = (torch.from_numpy(x[r].copy()).cuda() for x in (a, b, d))
            oa, ob, od = torch.zeros_like(ta), torch.zeros_like(tb), torch.zeros_like(td)
            collectives.allreduce(comm, ta, oa, "add")
            collectives.reduce(comm, tb, ob if r == 1 else None, "max", root=1)
            collectives.bcast(comm, ob, root=1)
            collectives.allreduce(comm, td, od, "min")
            s.synchronize()
        return oa.cpu().numpy(), ob.cpu().numpy(), od.cpu().numpy()

    want = (oracle_mod.reduce(a, FLOAT, ADD), oracle_mod.reduce(b, INT, MAX), oracle_mod.reduce(d, DOUBLE, MIN))
    for got in LocalGroup(n).run(fn):
        for g, w in zip(got, want):
            assert np.array_equal(g.view(np.uint8), w.view(np.uint8))


def test_allreduce_small_then_large_on_two_streams(gpu, oracle_mod, piece_bytes):
    """A small allreduce on stream A directly followed by a pipelined one on
    stream B, nothing between them on the host: both use the communicator's
    workspace, ordered through its stream."""
    from smi_amd import LocalGroup, collectives
    piece_bytes(65536)
    n = 4
    small = _contribs(oracle_mod, n, 60000, FLOAT, seed=5)
    large = _contribs(oracle_mod, n, 300001, FLOAT, seed=6)

    def fn(comm):
        sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
        ts = torch.from_numpy(small[comm.rank].copy()).cuda()
        tl = torch.from_numpy(large[comm.rank].copy()).cuda()
        os_, ol = torch.zeros_like(ts), torch.zeros_like(tl)
        torch.cuda.synchronize()
        outs = []
        for _ in range(3):
            collectives.allreduce(comm, ts, os_, "add", stream=sa)
            collectives.allreduce(comm, tl, ol, "add", stream=sb)
            sa.synchronize()
            sb.synchronize()
            outs.append((os_.cpu().numpy(), ol.cpu().numpy()))
            os_.zero_()
            ol.zero_()
            torch.cuda.synchronize()
        return outs

    ws, wl = oracle_mod.reduce(small, FLOAT, ADD), oracle_mod.reduce(large, FLOAT, ADD)
    for outs in LocalGroup(n).run(fn):
        for gs, gl in outs:
            assert np.array_equal(gs.view(np.uint32), ws.view(np.uint32))
            assert np.array_equal(gl.view(np.uint32), wl.view(np.uint32))


def test_allreduce_argument_errors(gpu):
    from smi_amd import LocalGroup, SMIError, _lib, collectives

    def fn(comm):
        x = torch.ones(16, device="cuda")
        y = torch.zeros(16, device="cuda")
        h = _lib.stream_handle(None)
        with pytest.raises(SMIError, match="bad op"):
            collectives.allreduce(comm, x, y, 3)
        with pytest.raises(SMIError, match="NULL recvbuf"):
            _lib.call("smi_allreduce", comm.handle, x.data_ptr(), None, 16, _lib.SMI_FLOAT, _lib.SMI_ADD, 0, h)
        with pytest.raises(SMIError, match="NULL sendbuf"):
            _lib.call("smi_allreduce", comm.handle, None, y.data_ptr(), 16, _lib.SMI_FLOAT, _lib.SMI_ADD, 0, h)
        with pytest.raises(SMIError, match="unsupported"):
            _lib.call("smi_allreduce", comm.handle, x.data_ptr(), y.data_ptr(), 16, 99, _lib.SMI_ADD, 0, h)
        with pytest.raises(SMIError, match="unsupported dtype"):
            collectives.allreduce(comm, x.half(), None, "add")
        with pytest.raises(SMIError):
            collectives.allreduce(comm, x, torch.zeros(15, device="cuda"), "add")
        # count == 0: success, nothing touched, NULL buffers allowed
        _lib.call("smi_allreduce", comm.handle, None, None, 0, _lib.SMI_FLOAT, _lib.SMI_ADD, 0, h)
        collectives.allreduce(comm, x[:0], y[:0], "add")
        torch.cuda.synchronize()
        return y.cpu().numpy()

    for got in LocalGroup(2).run(fn):
        assert (got == 0).all()
