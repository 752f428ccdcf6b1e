"""Jacobi solve to a tolerance on the GPU: the fused residual step
(smi_stencil_step_residual) and smi_stencil_solve.

Contract: the residual of a step is max |x_t - x_{t-1}| over the cells the
step writes -- one fp32 subtraction and fabs per cell, NaN if any difference
is NaN -- which is one well-defined fp32 value whatever the order, so every
check here is bit for bit against numpy's max(abs(a - b)) over two oracle
states (all NaNs equal), and the grid a solve returns is bit-identical to the
oracle after `steps` steps.  The expected stop of a solve is derived from the
oracle's residual sequence at the check points, never from a constant.
"""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
F32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def np_resid(new, old, mask=None):
    """numpy restatement of the residual contract."""
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.abs(np.asarray(new, dtype=F32) - np.asarray(old, dtype=F32))
    if mask is not None:
        d = d[mask]
    if d.size == 0:
        return F32(0)
    if np.isnan(d).any():
        return F32(np.nan)
    return F32(d.max())


def same_f32(got, want):
    got, want = F32(got), F32(want)
    if np.isnan(want):
        return bool(np.isnan(got))
    return got.view(np.uint32) == want.view(np.uint32)


def word_value(word):
    return word.cpu().numpy().view(np.float32)[0]


@pytest.fixture
def restore_settings(gpu):
    from smi_amd import stencil
    tune, fuse = stencil.get_tuning(), stencil.get_fusion()["steps_per_pass"]
    yield
    stencil.set_tuning(tune["rows_per_wave"], tune["rows_in_flight"], tune["nontemporal"], tune["overlap"])
    stencil.set_fusion(steps_per_pass=fuse)


def fused_step(grid, modes=(0, 0, 0, 0), halos=(None,) * 4, word=None, fill=None):
    """(out, residual word) of one step(..., residual=...)."""
    from smi_amd import stencil
    a = torch.from_numpy(np.ascontiguousarray(grid)).cuda()
    out = torch.empty_like(a) if fill is None else torch.full_like(a, fill)
    if word is None:
        word = torch.zeros(1, dtype=torch.int32, device="cuda")
    stencil.step(a, out, modes, halos, residual=word)
    torch.cuda.synchronize()
    return out.cpu().numpy(), word


def plain_step(grid):
    from smi_amd import stencil
    a = torch.from_numpy(np.ascontiguousarray(grid)).cuda()
    out = torch.empty_like(a)
    stencil.step(a, out)
    torch.cuda.synchronize()
    return out.cpu().numpy()


# ------------------------------------------------------------ fused step --
SHAPES = [(1, 4), (2, 4), (3, 8), (5, 12), (7, 260), (129, 260), (300, 1028)]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("init", ["edges", "uniform"])
def test_fused_step_matches_plain_step_and_numpy(gpu, oracle_mod, restore_settings, shape, init):
    from smi_amd import stencil
    X, Y = shape
    g = oracle_mod.init_edges(X, Y) if init == "edges" else oracle_mod.init_uniform(X, Y, seed=X * 31 + Y)
    want = oracle_mod.stencil(g, 1)
    want_r = np_resid(want, g)
    for rpw in (1, 7):
        for rif in (1, 4):
            stencil.set_tuning(rows_per_wave=rpw, rows_in_flight=rif)
            out, word = fused_step(g)
            got_r = word_value(word)
            print(shape, init, rpw, rif, "residual", got_r, "want", want_r)
            assert np.array_equal(bits(out), bits(plain_step(g))), (shape, rpw, rif)
            assert np.array_equal(bits(out), bits(want)), (shape, rpw, rif)
            assert same_f32(got_r, want_r), (shape, rpw, rif, got_r, want_r)


def _planted_positions():
    pos = []
    X = 40
    for Y, cs in ((260, (1, 255, 256, 258)), (300, (296, 297, 298, 299))):
        # 260 wide: columns 1, 255 | 256 (the strip boundary) and cols-2, in
        # the first and last interior row: beside all four tile corners too.
        # 300 wide: the partial strip's last lane (columns 296..299).
        for r in (1, X - 2):
            for c in cs:
                pos.append((X, Y, r, c))
    pos += [(X, 260, 17, 130), (X, 300, 0, 5), (X, 300, 20, 0)]   # mid-tile; on the copied edge
    return pos


@pytest.mark.parametrize("X,Y,r,c", _planted_positions())
def test_planted_maximum_is_found(gpu, oracle_mod, X, Y, r, c):
    g = oracle_mod.init_uniform(X, Y, seed=11)
    g[r, c] = F32(1000.0)
    want = oracle_mod.stencil(g, 1)
    want_r = np_resid(want, g)
    interior = 0 < r < X - 1 and 0 < c < Y - 1
    with np.errstate(invalid="ignore"):
        where = np.unravel_index(np.argmax(np.abs(want - g)), g.shape)
    if interior:
        assert where == (r, c) and want_r > 990      # the planted cell itself holds the maximum
    else:
        assert abs(where[0] - r) + abs(where[1] - c) == 1 and 240 < want_r < 260   # its one interior neighbour
    out, word = fused_step(g)
    assert np.array_equal(bits(out), bits(want))
    assert same_f32(word_value(word), want_r), (word_value(word), want_r)


# ------------------------------------------------------------ side modes --
def _ext_reference(oracle_mod, tile, halos, modes):
    """A step with halo vectors equals a full-grid step on the tile extended
    by its halo ring; COPY sides keep their input cells.  SKIP sides are
    computed like HALO sides here and masked out by the caller."""
    X, Y = tile.shape
    ext = np.zeros((X + 2, Y + 2), dtype=np.float32)
    ext[1:-1, 1:-1] = tile
    ext[0, 1:-1] = halos[0]
    ext[-1, 1:-1] = halos[1]
    ext[1:-1, 0] = halos[2]
    ext[1:-1, -1] = halos[3]
    ref = oracle_mod.stencil(ext, 1)[1:-1, 1:-1].copy()
    if modes[0] == 0:
        ref[0, :] = tile[0, :]
    if modes[1] == 0:
        ref[-1, :] = tile[-1, :]
    if modes[2] == 0:
        ref[:, 0] = tile[:, 0]
    if modes[3] == 0:
        ref[:, -1] = tile[:, -1]
    return ref


def _written_mask(shape, modes):
    m = np.ones(shape, dtype=bool)
    if modes[0] == 2:
        m[0, :] = False
    if modes[1] == 2:
        m[-1, :] = False
    if modes[2] == 2:
        m[:, 0] = False
    if modes[3] == 2:
        m[:, -1] = False
    return m


@pytest.mark.parametrize("modes", [(1, 1, 1, 1), (0, 1, 0, 1), (1, 0, 1, 0), (0, 0, 1, 1), (1, 1, 0, 0)])
@pytest.mark.parametrize("shape", [(1, 4), (6, 8), (70, 516)])
def test_halo_sides(gpu, oracle_mod, modes, shape):
    X, Y = shape
    rng = np.random.default_rng(X + Y)
    tile = rng.random((X, Y), dtype=np.float32)
    halos = [rng.random(Y, dtype=np.float32) * 3, rng.random(Y, dtype=np.float32) * 3,
             rng.random(X, dtype=np.float32) * 3, rng.random(X, dtype=np.float32) * 3]
    want = _ext_reference(oracle_mod, tile, halos, modes)
    hd = [torch.from_numpy(h).cuda() if m == 1 else None for h, m in zip(halos, modes)]
    out, word = fused_step(tile, modes, hd)
    assert np.array_equal(bits(out), bits(want))
    assert same_f32(word_value(word), np_resid(want, tile)), (word_value(word), np_resid(want, tile))


@pytest.mark.parametrize("modes", [(2, 2, 2, 2), (2, 0, 1, 2), (1, 2, 2, 0)])
@pytest.mark.parametrize("shape", [(6, 8), (40, 520)])
def test_skip_sides_do_not_contribute(gpu, oracle_mod, modes, shape):
    """The largest difference of the step sits in a skipped row and in a
    skipped column (huge halo values there, which only the skipped cells
    read): the residual is that of the written cells alone."""
    X, Y = shape
    tile = oracle_mod.init_uniform(X, Y, seed=3)
    rng = np.random.default_rng(5)
    halos = [rng.random(Y, dtype=np.float32), rng.random(Y, dtype=np.float32), rng.random(X, dtype=np.float32),
             rng.random(X, dtype=np.float32)]
    for k in range(4):
        if modes[k] == 2:
            halos[k][len(halos[k]) // 2] = F32(1e6)
    ref = _ext_reference(oracle_mod, tile, halos, modes)
    mask = _written_mask(tile.shape, modes)
    want_r = np_resid(ref, tile, mask)
    assert np_resid(ref, tile) > 1e5 and want_r < 10          # the planted differences are the largest by far
    hd = [torch.from_numpy(h).cuda() if m != 0 else None for h, m in zip(halos, modes)]
    out, word = fused_step(tile, modes, hd, fill=-7.0)
    assert np.array_equal(bits(out[mask]), bits(ref[mask]))
    assert (out[~mask] == -7).all()
    assert same_f32(word_value(word), want_r), (word_value(word), want_r)


def test_two_calls_accumulate_into_one_word(gpu, oracle_mod):
    small = oracle_mod.init_uniform(33, 264, seed=1)
    big = oracle_mod.init_uniform(9, 12, seed=2) * F32(64)
    r_small = np_resid(oracle_mod.stencil(small, 1), small)
    r_big = np_resid(oracle_mod.stencil(big, 1), big)
    assert r_big > r_small
    for first, second in ((small, big), (big, small)):
        _, word = fused_step(first)
        _, word = fused_step(second, word=word)
        assert same_f32(word_value(word), r_big)
    # a word that already holds more than both keeps its value
    word = torch.from_numpy(np.array([1e9], dtype=np.float32).view(np.int32)).cuda()
    _, word = fused_step(big, word=word)
    assert same_f32(word_value(word), F32(1e9))


# --------------------------------------------------------- special values --
def test_subnormal_differences_are_kept(gpu, oracle_mod):
    g = (oracle_mod.init_uniform(20, 264, seed=4).astype(np.float64) * 1e-40).astype(np.float32)
    want = oracle_mod.stencil(g, 1)
    want_r = np_resid(want, g)
    assert 0 < want_r < np.finfo(np.float32).tiny       # a subnormal, not flushed
    out, word = fused_step(g)
    assert np.array_equal(bits(out), bits(want))
    assert same_f32(word_value(word), want_r)


def test_negative_zero_gives_bits_zero(gpu, oracle_mod):
    """+0 cells among -0 neighbours: o = -0, c = +0, o - c = -0, whose sign
    fabs clears -- the word stays 0 (an uncleared sign bit would be the
    largest unsigned pattern)."""
    X, Y = 12, 264
    i, j = np.indices((X, Y))
    g = np.where((i + j) % 2 == 0, F32(0.0), F32(-0.0)).astype(np.float32)
    want = oracle_mod.stencil(g, 1)
    assert np.signbit(want - g).any()                   # there are -0 differences
    out, word = fused_step(g)
    assert np.array_equal(bits(out), bits(want))
    assert int(word.cpu().numpy()[0]) == 0


def test_nan_and_inf_cells(gpu, oracle_mod):
    """One NaN cell: NaN.  One inf cell: inf after step 1 and, by the oracle,
    inf again after step 2 -- the cells holding inf after step t all lie at a
    distance of t's parity from it, so no cell is inf in two consecutive
    states and inf - inf does not occur.  Two inf cells at an odd distance
    break that: inf after step 1, NaN (inf - inf) after step 2.  An inf cell
    on the copied global edge is inf - inf = NaN at once."""
    g = oracle_mod.init_uniform(20, 264, seed=6)
    g[7, 100] = np.nan
    _, word = fused_step(g)
    assert np.isnan(word_value(word))
    for cells, want2_nan in (([(9, 259)], False), ([(9, 100), (9, 103)], True)):
        g = oracle_mod.init_uniform(20, 264, seed=7)
        for rc in cells:
            g[rc] = np.inf
        x1 = oracle_mod.stencil(g, 1)
        x2 = oracle_mod.stencil(x1, 1)
        assert np.isposinf(np_resid(x1, g))
        assert np.isnan(np_resid(x2, x1)) == want2_nan and (want2_nan or np.isposinf(np_resid(x2, x1)))
        out1, w1 = fused_step(g)
        out2, w2 = fused_step(out1)
        assert same_f32(word_value(w1), np_resid(x1, g)), cells
        assert same_f32(word_value(w2), np_resid(x2, x1)), cells
        assert np.array_equal(np.isnan(out2), np.isnan(x2))
    g = oracle_mod.init_uniform(20, 264, seed=8)
    g[0, 77] = np.inf
    _, word = fused_step(g)
    assert np.isnan(np_resid(oracle_mod.stencil(g, 1), g)) and np.isnan(word_value(word))


# ------------------------------------------------------------------ solve --
def oracle_sequence(oracle_mod, g, T):
    """states x_0..x_T and residuals r_1..r_T (r[0] unused) of the oracle."""
    states, r = [np.ascontiguousarray(g, dtype=np.float32)], [None]
    for _ in range(T):
        nxt = oracle_mod.stencil(states[-1], 1)
        r.append(np_resid(nxt, states[-1]))
        states.append(nxt)
    return states, r


def expected_stop(r, tol, max_steps, check_every):
    """(steps, residual, converged) from the residuals at the check points."""
    t, last = 0, F32(np.inf)
    while t < max_steps:
        t = min(t + check_every, max_steps)
        last = r[t]
        if last <= F32(tol):
            return t, last, True
    return t, last, False


@pytest.fixture(scope="module")
def seq16(oracle_mod):
    from smi_amd import stencil
    return oracle_sequence(oracle_mod, stencil.init_grid(16, 32), 1500)


def run_solve(g, tol, max_steps, check_every):
    from smi_amd import LocalGroup, stencil
    comm = LocalGroup(1).comm(0)
    try:
        t = torch.from_numpy(np.ascontiguousarray(g)).cuda()
        res, steps, r, conv = stencil.solve(comm, t, tol, max_steps, check_every, 1, 1)
        torch.cuda.synchronize()
        return res.cpu().numpy(), steps, r, conv
    finally:
        comm.finalize()


@pytest.mark.parametrize("tol,check_every,max_steps", [
    (1e-3, 1, 600), (1e-3, 7, 600), (1e-3, 20, 600), (1e-3, 64, 600), (0.0, 1, 1500),
    (1e-3, 64, 250),    # last round shorter: check points 64, 128, 192, 250
    (1e-3, 64, 100),    # max_steps reached, also not a multiple
    (1e-3, 20, 200)])   # max_steps reached at a check point
def test_solve_single_tile(gpu, seq16, tol, check_every, max_steps):
    states, r = seq16
    steps_w, r_w, conv_w = expected_stop(r, tol, max_steps, check_every)
    got, steps, res, conv = run_solve(states[0], tol, max_steps, check_every)
    print("steps", steps, "want", steps_w, "residual", res, "want", r_w, "converged", conv)
    assert steps == steps_w
    assert same_f32(res, r_w), (res, r_w)
    assert conv == conv_w
    assert np.array_equal(bits(got), bits(states[steps]))


def test_solve_reference_sequence_shape(seq16):
    """What the cases above rely on: 1e-3 is first met well inside 600
    steps, the exact fixed point inside 1500, and not at the short limits."""
    _, r = seq16
    first = next(t for t in range(1, 1501) if r[t] <= F32(1e-3))
    fixed = next(t for t in range(1, 1501) if r[t] == 0)
    assert 200 < first < 250 and first < fixed < 1500


def test_solve_zero_steps_and_nan_grid(gpu, seq16):
    states, _ = seq16
    got, steps, res, conv = run_solve(states[0], 1e-3, 0, 5)
    assert steps == 0 and np.isposinf(res) and not conv
    assert np.array_equal(bits(got), bits(states[0]))
    g = states[0].copy()
    g[5, 9] = np.nan
    got, steps, res, conv = run_solve(g, 1e-3, 10, 3)
    assert steps == 10 and np.isnan(res) and not conv
    import oracle
    want = oracle.stencil(g, 10)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(bits(got)[~np.isnan(want)], bits(want)[~np.isnan(want)])


def test_solve_is_fusion_neutral(gpu, oracle_mod, restore_settings):
    """96x128, check_every = 41: the 40 unchecked steps between two checks
    run as two K = 20 passes under steps_per_pass = 20 (12: 10+10+10+10, 2:
    pairs, 1: single steps); steps, residual and grid never change."""
    from smi_amd import stencil
    g = oracle_mod.init_uniform(96, 128, seed=96)
    tol, ce, max_steps = 0.07, 41, 200      # a random grid smooths slowly: met at the third check
    r, states, x = {}, {}, g
    done = 0
    while done < max_steps:                 # oracle states at the check points only
        nxt = min(done + ce, max_steps)
        prev = oracle_mod.stencil(x, nxt - done - 1)
        x = oracle_mod.stencil(prev, 1)
        r[nxt], states[nxt] = np_resid(x, prev), x
        done = nxt
    steps_w = next((t for t in sorted(r) if r[t] <= F32(tol)), max_steps)
    assert sorted(r)[0] < steps_w < max_steps       # neither the first check nor the step limit
    stencil.set_fusion(steps_per_pass=20)
    assert stencil.plan(96, 128, 1, 1, 0, ce - 1)["phases"] == [(20, 2)]
    for k in (1, 2, 12, 20):
        stencil.set_fusion(steps_per_pass=k)
        got, steps, res, conv = run_solve(g, tol, max_steps, ce)
        print("K", k, "steps", steps, "want", steps_w, "residual", res, "want", r[steps_w])
        assert steps == steps_w, k
        assert same_f32(res, r[steps_w]), (k, res, r[steps_w])
        assert conv == bool(r[steps_w] <= F32(tol))
        assert np.array_equal(bits(got), bits(states[steps_w])), k


# ------------------------------------------------------ solve, decomposed --
def decomposed_solve(grid, PX, PY, overlap, tol, max_steps, check_every):
    from smi_amd import LocalGroup, stencil
    stencil.set_tuning(overlap=overlap)
    tiles = stencil.split_memory(grid, PX, PY)

    def rank_fn(comm):
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            t = torch.from_numpy(tiles[comm.rank]).cuda()
            res, steps, r, conv = stencil.solve(comm, t, tol, max_steps, check_every, PX, PY)
            s.synchronize()
            return res.cpu().numpy(), steps, r, conv

    try:
        out = LocalGroup(PX * PY).run(rank_fn)
    finally:
        stencil.set_tuning(overlap=1)
    return stencil.combine_memory([o[0] for o in out], PX, PY), [o[1:] for o in out]


@pytest.mark.parametrize("overlap", [0, 1])
@pytest.mark.parametrize("pxpy", [(2, 1), (1, 2), (2, 2), (2, 4)])
def test_solve_decomposed_matches_single_tile(gpu, oracle_mod, pxpy, overlap):
    from smi_amd import stencil
    PX, PY = pxpy
    tol, ce, max_steps = 1e-3, 20, 600
    g = stencil.init_grid(16 * PX, 32 * PY)
    states, r = oracle_sequence(oracle_mod, g, max_steps)
    steps_w, r_w, conv_w = expected_stop(r, tol, max_steps, ce)
    got, per_rank = decomposed_solve(g, PX, PY, overlap, tol, max_steps, ce)
    print(pxpy, overlap, "want", steps_w, r_w, "got", per_rank)
    for steps, res, conv in per_rank:
        assert steps == steps_w and same_f32(res, r_w) and conv == conv_w, (per_rank, steps_w, r_w)
    assert np.array_equal(bits(got), bits(states[steps_w]))


@pytest.mark.parametrize("pxpy", [(2, 2), (1, 2)])
def test_solve_residual_is_global_on_every_rank(gpu, oracle_mod, pxpy):
    """One spike deep inside one rank's tile of an otherwise constant grid:
    for three steps every other rank's own cells do not change at all, so a
    rank that used its local residual would report 0 and (tol = 0.5) stop."""
    PX, PY = pxpy
    XL, YL = 16, 32
    for owner in range(PX * PY):
        g = np.full((XL * PX, YL * PY), 0.5, dtype=np.float32)
        g[(owner // PY) * XL + 8, (owner % PY) * YL + 16] = F32(100.0)
        states, r = oracle_sequence(oracle_mod, g, 3)
        assert all(x > 1 for x in r[1:])
        steps_w, r_w, conv_w = expected_stop(r, 0.5, 3, 1)
        assert steps_w == 3 and not conv_w
        got, per_rank = decomposed_solve(g, PX, PY, 1, 0.5, 3, 1)
        for steps, res, conv in per_rank:
            assert steps == 3 and same_f32(res, r_w) and not conv, (owner, per_rank, r_w)
        assert np.array_equal(bits(got), bits(states[3]))


# ---------------------------------------------------- two RCCL processes --
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_solve_two_rccl_processes(gpu):
    """tests/solve_worker.py as two fresh child processes, one rank each,
    over the production transport: 1x2 and 2x1, 32x64 tiles, tol 1e-3,
    check_every 20, bit-exact against the oracle (the reduce/bcast pair and
    the halo exchanges stay ordered on one RCCL communicator)."""
    world = 2
    ngpu = torch.cuda.device_count()
    port = _free_port()
    procs = []
    for r in range(world):
        env = dict(os.environ)
        env.update(RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK=str(r % max(1, ngpu)),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
        if ngpu < world:
            env.update(NCCL_HOSTID=f"smi-test-host-{r}", NCCL_SOCKET_IFNAME="lo", NCCL_IB_DISABLE="1")
        procs.append(subprocess.Popen([sys.executable, "-u", os.path.join(HERE, "solve_worker.py")], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs, rcs = [], []
    for p in procs:
        try:
            out, _ = p.communicate(timeout=180)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            out, _ = p.communicate()
            out += "\n<killed: time limit>"
        outs.append(out)
        rcs.append(p.returncode)
    log = "\n".join(f"--- rank {r} (rc {rc})\n{o[-4000:]}" for r, (rc, o) in enumerate(zip(rcs, outs)))
    print(log)
    assert all(rc == 0 for rc in rcs), log
    assert "SOLVE MULTIPROC PASS" in outs[0], log
    assert sum(o.count(" CASE ") for o in outs) >= 4 and not any("MISMATCH" in o for o in outs), log
