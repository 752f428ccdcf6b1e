"""Multi-rank source runs with K-step passes (smi_stencil_set_source_bands(1)):
the source band kernel, the depth-K halos of g and the schedule around them.

The yardstick is np_step below, a numpy restatement of the header's contract
(float32 arrays, one ufunc per operation, g added last before the multiply,
global-edge cells copied) on the whole grid.  Every comparison is bit for bit,
NaNs compared as NaNs; nothing is compared with the library's own output.  Ranks
are LocalGroup threads on one GPU.  Every run also checks that `src` comes back
unchanged and that the result is the buffer stencil.plan(source=True) names.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

F32 = np.float32
TILE = (61, 140)        # odd rows; 140 columns end in a partial band segment for every K


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_grid(got, want):
    """bit-identical, all NaNs equal"""
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got)[~nan], bits(want)[~nan])


def np_step(a, g):
    """one step of the contract: interior 0.25 * ((((S + W) + E) + N) + g), edges copied"""
    a = np.asarray(a, dtype=F32)
    o = a.copy()
    with np.errstate(all="ignore"):
        o[1:-1, 1:-1] = F32(0.25) * ((((a[2:, 1:-1] + a[1:-1, :-2]) + a[1:-1, 2:]) + a[:-2, 1:-1]) + g[1:-1, 1:-1])
    return o


def np_run(a, g, T):
    for _ in range(T):
        a = np_step(a, g)
    return np.asarray(a, dtype=F32)


def np_resid(new, old):
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.abs(np.asarray(new, dtype=F32) - np.asarray(old, dtype=F32))
    return F32(np.nan) if np.isnan(d).any() else F32(d.max())


def uniform(shape, seed, lo=-0.5):
    return (np.random.default_rng(seed).random(shape, dtype=np.float32) + F32(lo)).astype(np.float32)


def kc_of(K):
    return 4 * ((K + 3) // 4)


@pytest.fixture(scope="module")
def KS(gpu):
    from smi_amd import stencil
    return stencil.source_max_depth()


@pytest.fixture(autouse=True)
def restore_settings(gpu):
    """source bands on for the test; the switch, fusion, bands, join and tuning restored after it"""
    from smi_amd import stencil
    switch, tune, fuse = stencil.get_source_bands(), stencil.get_tuning(), stencil.get_fusion()["steps_per_pass"]
    bands, join = stencil.get_bands(), stencil.get_join()
    stencil.set_fusion(steps_per_pass=12)
    htk = stencil.get_fusion()["rows_per_wave"]          # the K-step sweep's rows per wave (0: automatic)
    stencil.set_fusion(steps_per_pass=fuse)
    stencil.set_source_bands(1)
    yield
    stencil.set_source_bands(switch)
    stencil.set_tuning(tune["rows_per_wave"], tune["rows_in_flight"], tune["nontemporal"], tune["overlap"])
    stencil.set_bands(bands["reserve_waves"], bands["interior_rounds"])
    stencil.set_join(join)
    stencil.set_fusion(steps_per_pass=12, rows_per_wave=htk if htk > 0 else -1)
    stencil.set_fusion(steps_per_pass=fuse)


def decomposed_run(grid, g, PX, PY, T, overlap=1, priority=0, phases=None):
    """smi_stencil_run_source on PX x PY LocalGroup ranks; the combined grid.
    phases: the schedule every rank must report."""
    from smi_amd import LocalGroup, stencil
    stencil.set_tuning(overlap=overlap)
    tiles, srcs = stencil.split_memory(grid, PX, PY), stencil.split_memory(g, PX, PY)

    def rank_fn(comm):
        s = torch.cuda.Stream(priority=priority)
        with torch.cuda.stream(s):
            t = torch.from_numpy(np.array(tiles[comm.rank])).cuda()          # (writable copies)
            src = torch.from_numpy(np.array(srcs[comm.rank])).cuda()
            scratch = torch.full_like(t, -7.0)
            p = stencil.plan(*t.shape, PX, PY, comm.rank, T, source=True)
            res = stencil.run(comm, t, T, PX, PY, scratch=scratch, source=src)
            s.synchronize()
            assert res is (t, scratch)[p["result_index"]], (comm.rank, p)
            assert same_grid(src.cpu().numpy(), srcs[comm.rank]), comm.rank          # src is never written
            return res.cpu().numpy(), p["phases"]

    try:
        out = LocalGroup(PX * PY).run(rank_fn)
    finally:
        stencil.set_tuning(overlap=1)
    if phases is not None:
        assert all(ph == phases for _, ph in out), [ph for _, ph in out]
    return stencil.combine_memory([o[0] for o in out], PX, PY)


_STATES = {}


def states_of(shape, steps=23):
    """numpy states x_0..x_steps of a uniform grid in [-0.5, 0.5) under a uniform source, once per module"""
    if shape not in _STATES:
        a, g = uniform(shape, shape[0] * 31 + shape[1]), uniform(shape, shape[0] + 7 * shape[1])
        st = [a]
        for _ in range(steps):
            st.append(np_step(st[-1], g))
        for s in st + [g]:
            s.setflags(write=False)
        _STATES[shape] = (st, g)
    return _STATES[shape]


# --------------------------------------------------------- 1. every depth --
def test_the_depths_below_are_all_of_them(KS):
    assert list(range(3, 10)) == list(range(3, KS + 1))


@pytest.mark.parametrize("K", range(3, 10))
@pytest.mark.parametrize("pxpy", [(2, 1), (1, 2), (2, 2), (3, 3)])
def test_every_depth(KS, pxpy, K):
    """T = K, 2K + 1 (K-step passes + one single step) and 2K + 5 (two phase
    depths at K = 6, 7 and 9, where 2K + 5 is no multiple of the pass count), with and
    without overlap.  (3, 3) has a rank with eight neighbours."""
    from smi_amd import stencil
    assert K <= KS
    PX, PY = pxpy
    st, g = states_of((TILE[0] * PX, TILE[1] * PY))
    stencil.set_fusion(steps_per_pass=K, rows_per_wave=-1)
    assert stencil.plan(*TILE, PX, PY, 0, 2 * K + 1, source=True)["phases"] == [(K, 2), (1, 1)]
    if K in (6, 7, 9):
        ph = stencil.plan(*TILE, PX, PY, 0, 2 * K + 5, source=True)["phases"]
        assert len(ph) == 2 and all(3 <= s <= K for s, _ in ph), ph
    for T in (K, 2 * K + 1, 2 * K + 5):
        for overlap in (0, 1):
            got = decomposed_run(st[0], g, PX, PY, T, overlap)
            assert np.array_equal(bits(got), bits(st[T])), (pxpy, K, T, overlap)


# ------------------------------------------------------- 2. smallest tiles --
@pytest.mark.parametrize("kk", ["4", "8", "KS"])
def test_smallest_tiles(KS, kk):
    """Tiles of exactly 2K x 2KC on a 2 x 3 grid: the bands are the whole tile."""
    from smi_amd import stencil
    K = KS if kk == "KS" else int(kk)
    X, Y = 2 * K, 2 * kc_of(K)
    st, g = states_of((2 * X, 3 * Y))
    stencil.set_fusion(steps_per_pass=K, rows_per_wave=-1)
    for T, ph in ((K, [(K, 1)]), (2 * K + 1, [(K, 2), (1, 1)])):
        for overlap in (0, 1):
            got = decomposed_run(st[0], g, 2, 3, T, overlap, phases=ph)
            assert np.array_equal(bits(got), bits(st[T])), (K, T, overlap)


def test_tiles_that_clip_the_depth(KS):
    """10 x 16 tiles hold K <= 5 whatever the fusion setting."""
    from smi_amd import stencil
    st, g = states_of((20, 48))
    stencil.set_fusion(steps_per_pass=KS, rows_per_wave=-1)
    for T, ph in ((5, [(5, 1)]), (11, [(5, 2), (1, 1)]), (15, [(5, 3)]), (9, [(5, 1), (4, 1)])):
        got = decomposed_run(st[0], g, 2, 3, T, phases=ph)
        assert np.array_equal(bits(got), bits(st[T])), T


# ----------------------------------------------------- 3. ring phase of g --
@pytest.mark.parametrize("K", range(3, 10))
def test_ring_phase_of_g(KS, K):
    """g[i][j] = 1000 i + j (exact in fp32) on a zero grid: a g halo that is off
    by a row, a column, a corner block or a transposition gives other bits."""
    from smi_amd import stencil
    assert K <= KS
    shape = (3 * TILE[0], 3 * TILE[1])
    i, j = np.indices(shape)
    g = (1000.0 * i + j).astype(np.float32)
    assert np.array_equal(g.astype(np.int64), 1000 * i + j)
    a = np.zeros(shape, dtype=np.float32)
    stencil.set_fusion(steps_per_pass=K, rows_per_wave=-1)
    for T in (K, 2 * K + 5):
        assert np.array_equal(bits(decomposed_run(a, g, 3, 3, T)), bits(np_run(a, g, T))), (K, T)


# -------------------------------------------------- 4. single source cell --
def _cell_cases(K):
    X, Y = TILE        # seams of the (3, 3) grid: rows X, 2X; columns Y, 2Y; rank 4 is the centre
    return [("last_row_above_seam", (X - 1, Y + 60)), ("first_row_below_seam", (X, Y + 60)),
            ("last_col_left_of_seam", (X + 30, Y - 1)), ("first_col_right_of_seam", (X + 30, Y)),
            ("corner_of_rank_0", (X - 1, Y - 1)), ("corner_of_rank_8", (2 * X, 2 * Y)),
            ("k_minus_1_rows_below_seam", (X + K - 1, Y + 70)), ("k_minus_1_cols_left_of_seam", (X + 30, 2 * Y - K))]


@pytest.mark.parametrize("which", range(8))
@pytest.mark.parametrize("kk", ["3", "KS"])
def test_single_source_cell(KS, kk, which):
    from smi_amd import stencil
    K = 3 if kk == "3" else KS
    name, cell = _cell_cases(K)[which]
    shape = (3 * TILE[0], 3 * TILE[1])
    g = np.zeros(shape, dtype=np.float32)
    g[cell] = F32(3.0e6)
    a = np.zeros(shape, dtype=np.float32)
    stencil.set_fusion(steps_per_pass=K, rows_per_wave=-1)
    for T in (K, K + 1):
        want = np_run(a, g, T)
        assert want[cell] != 0
        assert np.array_equal(bits(decomposed_run(a, g, 3, 3, T)), bits(want)), (name, K, T)


# ---------------------------------------------------------------- 5. g = -0 --
@pytest.mark.parametrize("kk", ["3", "KS"])
def test_minus_zero_source_is_the_plain_update(oracle_mod, KS, kk):
    from smi_amd import stencil
    K = 3 if kk == "3" else KS
    X, Y = 2 * TILE[0], 2 * TILE[1]
    a = oracle_mod.init_uniform(X, Y, seed=X + Y).copy()
    a[TILE[0] - 4:TILE[0] + 5, TILE[1] - 4:TILE[1] + 5] = F32(-0.0)       # across both seams
    a[X // 4:X // 4 + 9, 2:11] = F32(-0.0)
    a[X - 6:X - 1, Y - 6:Y - 1] = F32(-0.0)
    g = np.full((X, Y), -0.0, dtype=np.float32)
    want = oracle_mod.stencil(a, 25)
    assert np.array_equal(bits(np_run(a, g, 25)), bits(want))          # the restatement agrees with the oracle
    stencil.set_fusion(steps_per_pass=K, rows_per_wave=-1)
    assert np.array_equal(bits(decomposed_run(a, g, 2, 2, 25)), bits(want)), K


# ------------------------------------------------------ 6. NaN on the edge --
@pytest.mark.parametrize("kk", ["3", "KS"])
@pytest.mark.parametrize("pxpy", [(2, 2), (3, 3)])
def test_nan_on_the_global_edge_of_src_does_not_leak(KS, pxpy, kk):
    from smi_amd import stencil
    fuse = 3 if kk == "3" else KS
    PX, PY = pxpy
    st, g0 = states_of((TILE[0] * PX, TILE[1] * PY))
    g0 = g0.copy()
    g0[0, :] = g0[-1, :] = g0[:, 0] = g0[:, -1] = 0
    gn = g0.copy()
    gn[0, :] = gn[-1, :] = gn[:, 0] = gn[:, -1] = np.nan
    stencil.set_fusion(steps_per_pass=fuse, rows_per_wave=-1)
    T = 2 * fuse + 1
    want = np_run(st[0], g0, T)
    for overlap in (0, 1):
        got = decomposed_run(st[0], gn, PX, PY, T, overlap)
        assert not np.isnan(got).any()
        assert np.array_equal(bits(got), bits(want)), (pxpy, fuse, overlap)


# ------------------------------------------------------------- 7. specials --
def test_special_values(KS):
    from smi_amd import stencil
    K = KS
    X, Y = TILE
    shape = (2 * X, 2 * Y)
    stencil.set_fusion(steps_per_pass=K, rows_per_wave=-1)
    base_a, base_g = uniform(shape, 6), uniform(shape, 8)
    tiny = F32(1e-40)
    assert 0 < tiny < np.finfo(np.float32).tiny
    seam_cells = [(X - 1, Y + 20), (X + 10, Y)]          # above the horizontal seam, right of the vertical one
    for sval in (F32(np.inf), F32(np.nan), tiny):
        g = base_g.copy()
        for cell in seam_cells:
            g[cell] = sval
        for T in (K, K + 2):
            assert same_grid(decomposed_run(base_a, g, 2, 2, T), np_run(base_a, g, T)), (sval, T)
    for aval in (F32(1e35), F32(1e-36)):
        a = base_a.copy()
        for cell in seam_cells:
            a[cell] = aval
        assert same_grid(decomposed_run(a, base_g, 2, 2, K), np_run(a, base_g, K)), aval


# ------------------------------------------------- 8. scheduling settings --
@pytest.mark.parametrize("kk", ["3", "7", "KS"])
def test_scheduling_settings_are_bit_neutral(KS, kk):
    from smi_amd import stencil
    K = KS if kk == "KS" else int(kk)
    st, g = states_of((3 * TILE[0], 3 * TILE[1]))
    stencil.set_fusion(steps_per_pass=K, rows_per_wave=-1)
    T = 2 * K + 1
    for reserve, rounds in ((0, 1), (64, 1), (65536, 1)):
        stencil.set_bands(reserve, rounds)
        assert np.array_equal(bits(decomposed_run(st[0], g, 3, 3, T)), bits(st[T])), (K, reserve)
    stencil.set_bands(0, 1)
    for join in (0, 1):
        stencil.set_join(join)
        assert np.array_equal(bits(decomposed_run(st[0], g, 3, 3, T)), bits(st[T])), (K, "join", join)
    stencil.set_join(1)
    # the caller's stream at normal priority (joined to the communicator's interior stream) and at the highest
    for priority in (0, -1):
        assert np.array_equal(bits(decomposed_run(st[0], g, 3, 3, T, priority=priority)), bits(st[T])), (K, priority)


# ---------------------------------------------------- 9. switch 0 / switch 1 --
@pytest.mark.parametrize("pxpy", [(2, 2), (3, 3)])
def test_both_switch_settings_give_the_same_grid(KS, pxpy):
    from smi_amd import stencil
    PX, PY = pxpy
    st, g = states_of((TILE[0] * PX, TILE[1] * PY))
    stencil.set_fusion(steps_per_pass=KS, rows_per_wave=-1)
    T = 2 * KS + 5
    stencil.set_source_bands(0)
    off = decomposed_run(st[0], g, PX, PY, T, phases=[(1, T)])
    stencil.set_source_bands(1)
    on = decomposed_run(st[0], g, PX, PY, T)
    assert np.array_equal(bits(off), bits(st[T])) and np.array_equal(bits(on), bits(st[T]))


# ----------------------------------------------------------------- 10. solve --
def test_solve_source_2x2_fused(oracle_mod, KS):
    """64x96, init_edges, source 0.01 uniform (seed 3), tol 1e-3, check every 8:
    the numpy loop with the same check points; the runs between them are one
    7-step pass on every rank."""
    from smi_amd import LocalGroup, stencil
    a = oracle_mod.init_edges(64, 96)
    g = (F32(0.01) * oracle_mod.init_uniform(64, 96, seed=3)).astype(np.float32)
    tol, ce, max_steps = 1e-3, 8, 4000
    x, steps_w, r_w = a, 0, F32(np.inf)
    while steps_w < max_steps:
        prev = np_run(x, g, ce - 1)
        x = np_step(prev, g)
        steps_w += ce
        r_w = np_resid(x, prev)
        if r_w <= F32(tol):
            break
    assert 8 < steps_w < max_steps and r_w <= F32(tol)
    stencil.set_fusion(steps_per_pass=KS, rows_per_wave=-1)
    assert stencil.plan(32, 48, 2, 2, 0, ce - 1, source=True)["phases"] == [(ce - 1, 1)]
    tiles, srcs = stencil.split_memory(a, 2, 2), stencil.split_memory(g, 2, 2)

    def rank_fn(comm):
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            t = torch.from_numpy(tiles[comm.rank]).cuda()
            src = torch.from_numpy(srcs[comm.rank]).cuda()
            res, steps, r, conv = stencil.solve(comm, t, tol, max_steps, ce, 2, 2, source=src)
            s.synchronize()
            return res.cpu().numpy(), steps, r, conv

    out = LocalGroup(4).run(rank_fn)
    for _, steps, r, conv in out:
        print("steps", steps, "want", steps_w, "residual", r, "want", r_w)
        assert steps == steps_w and conv and F32(r).view(np.uint32) == r_w.view(np.uint32), (steps, r)
    assert np.array_equal(bits(stencil.combine_memory([o[0] for o in out], 2, 2)), bits(x))


# ------------------------------------------------------------------ 11. plan --
@pytest.mark.parametrize("fuse,T", [(1, 5), (3, 7), (5, 13), (20, 20), (20, 41), (2, 4)])
def test_plan_names_the_result_tensor(KS, fuse, T):
    """decomposed_run checks on every rank that the run returns the buffer the
    plan names; here over schedules with an even and an odd number of passes."""
    from smi_amd import stencil
    stencil.set_fusion(steps_per_pass=fuse, rows_per_wave=-1)
    st, g = states_of((2 * TILE[0], 2 * TILE[1]), steps=23)
    p = stencil.plan(*TILE, 2, 2, 0, T, source=True)
    assert p["result_index"] == sum(n for _, n in p["phases"]) % 2
    want = st[T] if T <= 23 else np_run(st[23], g, T - 23)
    got = decomposed_run(st[0], g, 2, 2, T, phases=p["phases"])
    assert np.array_equal(bits(got), bits(want)), (fuse, T)
