"""Jacobi with a source term on the GPU: smi_stencil_step_source,
smi_stencil_run_source and smi_stencil_solve_source.

The yardstick is np_step below, a numpy restatement of the header's contract
(float32 arrays, one ufunc per operation, g added last before the multiply,
global-edge cells copied).  Every comparison is bit for bit, NaNs compared as
NaNs; nothing is compared with the library's own output.  g = -0.0 ties the new
kernels to the CPU oracle of the plain update: x + (-0) = x for every x.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

F32 = np.float32
SHAPES = [(26, 8), (40, 260), (40, 300), (129, 516)]


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


def np_resid(new, old, mask=None):
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


# the sweep's window geometry (smi_amd/csrc/stencilk.h): output columns per 256-column window
def window_cols(K):
    return 256 - 8 * (4 if K >= 9 else (K + 3) // 4)


@pytest.fixture(scope="module")
def KS(gpu):
    from smi_amd import stencil
    return stencil.source_max_depth()


@pytest.fixture
def restore_settings(gpu):
    from smi_amd import stencil
    tune, fuse = stencil.get_tuning(), stencil.get_fusion()["steps_per_pass"]
    stencil.set_fusion(steps_per_pass=12)
    htk = stencil.get_fusion()["rows_per_wave"]          # the K-step sweep's rows per wave (0: automatic)
    stencil.set_fusion(steps_per_pass=fuse)
    yield
    stencil.set_tuning(tune["rows_per_wave"], tune["rows_in_flight"], tune["nontemporal"], tune["overlap"])
    stencil.set_fusion(steps_per_pass=12, rows_per_wave=htk if htk > 0 else -1)
    stencil.set_fusion(steps_per_pass=fuse)


@pytest.fixture(scope="module")
def comm1(gpu):
    from smi_amd import LocalGroup
    comm = LocalGroup(1).comm(0)
    yield comm
    comm.finalize()


def run_source(comm, grid, g, T):
    from smi_amd import stencil
    t = torch.from_numpy(np.array(grid, dtype=np.float32)).cuda()
    src = torch.from_numpy(np.array(g, dtype=np.float32)).cuda()
    res = stencil.run(comm, t, T, 1, 1, source=src)
    torch.cuda.synchronize()
    assert same_grid(src.cpu().numpy(), np.asarray(g, dtype=F32))          # src is never written
    return res.cpu().numpy()


def uniform(shape, seed, lo=-0.5):
    return (np.random.default_rng(seed).random(shape, dtype=np.float32) + F32(lo)).astype(np.float32)


_STATES = {}


def states_of(shape):
    """numpy states x_0..x_23 of a uniform grid in [-0.5, 0.5) under a uniform source, once per module"""
    if shape not in _STATES:
        a, g = uniform(shape, shape[0] * 31 + shape[1]), uniform(shape, shape[0] + 7 * shape[1])
        st = [a]
        for _ in range(23):
            st.append(np_step(st[-1], g))
        for s in st + [g]:
            s.setflags(write=False)
        _STATES[shape] = (st, g)
    return _STATES[shape]


# ---------------------------------------------------------- 1. single step --
def source_step(grid, g, modes=(0, 0, 0, 0), halos=(None,) * 4, resid=False, fill=None, sends=False):
    from smi_amd import stencil
    a = torch.from_numpy(np.array(grid, dtype=np.float32)).cuda()        # (writable copies: the shared states are not)
    src = torch.from_numpy(np.array(g, dtype=np.float32)).cuda()
    out = torch.empty_like(a) if fill is None else torch.full_like(a, fill)
    word = torch.zeros(1, dtype=torch.int32, device="cuda") if resid else None
    sl = torch.full((grid.shape[0],), -3.0, device="cuda") if sends else None
    sr = torch.full((grid.shape[0],), -3.0, device="cuda") if sends else None
    stencil.step(a, out, modes, halos, send_left=sl, send_right=sr, residual=word, source=src)
    torch.cuda.synchronize()
    return (out.cpu().numpy(), word, None if sl is None else sl.cpu().numpy(),
            None if sr is None else sr.cpu().numpy())


def ext_reference(tile, g, halos, modes):
    """A step with halo vectors is a full-grid step on the tile extended by its
    halo ring (the ring's own g never reaches a result); COPY sides keep their
    input cells; SKIP sides are computed like HALO sides and masked by the caller."""
    X, Y = tile.shape
    ext = np.zeros((X + 2, Y + 2), dtype=np.float32)
    gx = np.zeros((X + 2, Y + 2), dtype=np.float32)
    ext[1:-1, 1:-1], gx[1:-1, 1:-1] = tile, g
    ext[0, 1:-1], ext[-1, 1:-1], ext[1:-1, 0], ext[1:-1, -1] = halos
    ref = np_step(ext, gx)[1:-1, 1:-1].copy()
    if modes[0] == 0:
        ref[0, :] = tile[0, :]
    if modes[1] == 0:
        ref[-1, :] = tile[-1, :]
    if modes[2] == 0:
        ref[:, 0] = tile[:, 0]
    if modes[3] == 0:
        ref[:, -1] = tile[:, -1]
    return ref


def written_mask(shape, modes):
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


# rows per wave / rows in flight: every instantiation of the source step (16 in flight runs as 8)
TUNINGS = [(12, 16), (7, 4), (1, 1), (5, 2)]


@pytest.mark.parametrize("shape", SHAPES)
def test_step_all_copy_sides(gpu, restore_settings, shape):
    from smi_amd import stencil
    st, g = states_of(shape)
    want = np_step(st[0], g)
    assert np.array_equal(bits(want), bits(st[1]))
    for rpw, rif in TUNINGS:
        stencil.set_tuning(rows_per_wave=rpw, rows_in_flight=rif)
        for resid in (False, True):
            out, word, _, _ = source_step(st[0], g, resid=resid)
            assert np.array_equal(bits(out), bits(want)), (shape, rpw, rif, resid)
            if resid:
                assert same_f32(word_value(word), np_resid(want, st[0])), (shape, rpw, rif)


@pytest.mark.parametrize("modes", [(1, 1, 1, 1), (0, 1, 0, 1), (1, 0, 1, 0)])
@pytest.mark.parametrize("shape", SHAPES)
def test_step_halo_sides_and_sends(gpu, restore_settings, shape, modes):
    from smi_amd import stencil
    X, Y = shape
    st, g = states_of(shape)
    rng = np.random.default_rng(X + Y)
    halos = [rng.random(Y, dtype=np.float32) * 3, rng.random(Y, dtype=np.float32) * 3,
             rng.random(X, dtype=np.float32) * 3, rng.random(X, dtype=np.float32) * 3]
    want = ext_reference(st[0], g, halos, modes)
    hd = [torch.from_numpy(h).cuda() if m == 1 else None for h, m in zip(halos, modes)]
    for rpw, rif in TUNINGS[:2]:
        stencil.set_tuning(rows_per_wave=rpw, rows_in_flight=rif)
        for resid in (False, True):
            out, word, sl, sr = source_step(st[0], g, modes, hd, resid=resid, sends=True)
            assert np.array_equal(bits(out), bits(want)), (shape, modes, resid)
            assert np.array_equal(bits(sl), bits(want[:, 0])) and np.array_equal(bits(sr), bits(want[:, -1]))
            if resid:
                assert same_f32(word_value(word), np_resid(want, st[0])), (shape, modes)


@pytest.mark.parametrize("modes", [(2, 2, 2, 2), (2, 0, 1, 2), (1, 2, 2, 0)])
@pytest.mark.parametrize("shape", SHAPES)
def test_step_skip_sides_left_unwritten(gpu, restore_settings, shape, modes):
    X, Y = shape
    st, g = states_of(shape)
    rng = np.random.default_rng(5)
    halos = [rng.random(Y, dtype=np.float32), rng.random(Y, dtype=np.float32), rng.random(X, dtype=np.float32),
             rng.random(X, dtype=np.float32)]
    ref = ext_reference(st[0], g, halos, modes)
    mask = written_mask(shape, modes)
    hd = [torch.from_numpy(h).cuda() if m != 0 else None for h, m in zip(halos, modes)]
    for resid in (False, True):
        out, word, _, _ = source_step(st[0], g, modes, hd, resid=resid, fill=-7.0)
        assert np.array_equal(bits(out[mask]), bits(ref[mask]))
        assert (out[~mask] == -7).all()
        if resid:
            assert same_f32(word_value(word), np_resid(ref, st[0], mask))


# ------------------------------------------------- 2. g = -0 and g = +0 --
def minus_zero_grid(oracle_mod, shape):
    X, Y = shape
    a = oracle_mod.init_uniform(X, Y, seed=X + Y).copy()
    a[X // 3:X // 3 + 9, 2:min(11, Y - 1)] = F32(-0.0)       # 9 x 9 where the grid is wide enough
    a[X - 6:X - 1, Y - 6:Y - 1] = F32(-0.0)
    return a


@pytest.mark.parametrize("shape", SHAPES)
def test_minus_zero_source_is_the_plain_update(gpu, oracle_mod, comm1, restore_settings, KS, shape):
    from smi_amd import stencil
    a = minus_zero_grid(oracle_mod, shape)
    g = np.full(shape, -0.0, dtype=np.float32)
    for T in (25, 1):
        want = oracle_mod.stencil(a, T)
        assert np.array_equal(bits(np_run(a, g, T)), bits(want))          # the restatement agrees with the oracle
        for fuse in (1, 3, KS, 20):
            stencil.set_fusion(steps_per_pass=fuse, rows_per_wave=-1)
            assert np.array_equal(bits(run_source(comm1, a, g, T)), bits(want)), (shape, fuse, T)


@pytest.mark.parametrize("shape", SHAPES[1:])
def test_plus_zero_source_is_not(gpu, oracle_mod, comm1, restore_settings, KS, shape):
    from smi_amd import stencil
    a = minus_zero_grid(oracle_mod, shape)
    g = np.zeros(shape, dtype=np.float32)
    want, plain = np_step(a, g), oracle_mod.stencil(a, 1)
    diff = bits(want) != bits(plain)
    assert diff.any() and (plain[diff] == 0).all() and np.signbit(plain[diff]).all()   # the cells whose sum is -0
    out, _, _, _ = source_step(a, g)
    assert np.array_equal(bits(out), bits(want))
    for fuse in (1, KS):
        stencil.set_fusion(steps_per_pass=fuse, rows_per_wave=-1)
        assert np.array_equal(bits(run_source(comm1, a, g, 1)), bits(want))
        want3 = np_run(a, g, 3)
        assert not np.array_equal(bits(want3), bits(oracle_mod.stencil(a, 3)))
        assert np.array_equal(bits(run_source(comm1, a, g, 3)), bits(want3)), (shape, fuse)


# ------------------------------------------------------ 3. every K in 3..KS --
@pytest.mark.parametrize("shape", SHAPES)
def test_every_depth(gpu, comm1, restore_settings, KS, shape):
    """K = 3 .. KS, T = K, K + 1 and 2K + 5; rows per wave automatic and 40:
    (129, 516) then runs four row blocks, the upward-walking bottom block and
    three strips."""
    from smi_amd import stencil
    st, g = states_of(shape)
    for K in range(3, KS + 1):
        for rpw in (-1, 40):
            stencil.set_fusion(steps_per_pass=K, rows_per_wave=rpw)
            assert stencil.plan(*shape, 1, 1, 0, K, source=True)["phases"] == [(K, 1)]
            for T in (K, K + 1, 2 * K + 5):
                got = run_source(comm1, st[0], g, T)
                assert np.array_equal(bits(got), bits(st[T])), (K, shape, rpw, T)


# ---------------------------------------------------------- 4. ring phase --
@pytest.mark.parametrize("shape", [(40, 300), (129, 516)])
def test_ring_phase(gpu, comm1, restore_settings, KS, shape):
    """g[i][j] = 1000 i + j (exact in fp32) on a zero grid: a g ring that is off
    by one row, one lane, or mirrored in the upward walk gives other bits after
    the first pass."""
    from smi_amd import stencil
    i, j = np.indices(shape)
    g = (1000.0 * i + j).astype(np.float32)
    assert np.array_equal(g.astype(np.int64), 1000 * i + j)
    a = np.zeros(shape, dtype=np.float32)
    for K in range(3, KS + 1):
        want = {T: np_run(a, g, T) for T in (K, 2 * K + 5)}
        for rpw in (-1, 40):
            stencil.set_fusion(steps_per_pass=K, rows_per_wave=rpw)
            for T in (K, 2 * K + 5):
                assert np.array_equal(bits(run_source(comm1, a, g, T)), bits(want[T])), (K, shape, rpw, T)


# -------------------------------------------------- 5. single source cell --
def _cell_cases(K):
    sw = window_cols(K)
    return [("first_row", (1, 200)), ("last_row", (127, 301)), ("first_col", (50, 1)), ("last_col", (77, 514)),
            ("window0_last_col", (20, sw - 1)), ("window1_first_col", (21, sw)),
            ("above_block_seam", (63, 100)), ("below_block_seam", (64, 300))]


@pytest.mark.parametrize("which", range(8))
@pytest.mark.parametrize("kk", ["3", "KS"])
def test_single_source_cell(gpu, comm1, restore_settings, KS, kk, which):
    """(129, 516) at 40 rows per wave: row blocks start at 0, 32, 64, 96."""
    from smi_amd import stencil
    K = 3 if kk == "3" else KS
    name, cell = _cell_cases(K)[which]
    shape = (129, 516)
    g = np.zeros(shape, dtype=np.float32)
    g[cell] = F32(3.0e6)
    a = np.zeros(shape, dtype=np.float32)
    stencil.set_fusion(steps_per_pass=K, rows_per_wave=40)
    for T in (K, K + 1):
        want = np_run(a, g, T)
        assert want[cell] != 0
        assert np.array_equal(bits(run_source(comm1, a, g, T)), bits(want)), (name, K, T)


# ------------------------------------------------------ 6. NaN on the edge --
@pytest.mark.parametrize("shape", SHAPES)
def test_nan_on_the_global_edge_of_src_does_not_leak(gpu, comm1, restore_settings, KS, shape):
    from smi_amd import stencil
    st, g0 = states_of(shape)
    g0 = g0.copy()
    g0[0, :] = g0[-1, :] = g0[:, 0] = g0[:, -1] = 0
    gn = g0.copy()
    gn[0, :] = gn[-1, :] = gn[:, 0] = gn[:, -1] = np.nan
    out, word, _, _ = source_step(st[0], gn, resid=True)
    want1 = np_step(st[0], g0)
    assert np.array_equal(bits(out), bits(want1)) and same_f32(word_value(word), np_resid(want1, st[0]))
    for fuse in (1, 3, KS):
        for rpw in (-1, 40):
            stencil.set_fusion(steps_per_pass=fuse, rows_per_wave=rpw)
            T = 2 * fuse + 1
            want = np_run(st[0], g0, T)
            got = run_source(comm1, st[0], gn, T)
            assert not np.isnan(got).any()
            assert np.array_equal(bits(got), bits(want)), (shape, fuse, rpw)


# ------------------------------------------------------------- 7. specials --
@pytest.mark.parametrize("kk", ["3", "KS"])
def test_special_values(gpu, comm1, restore_settings, KS, kk):
    from smi_amd import stencil
    K = 3 if kk == "3" else KS
    shape = (40, 264)
    stencil.set_fusion(steps_per_pass=K, rows_per_wave=-1)
    base_a, base_g = uniform(shape, 6), uniform(shape, 8)
    tiny = F32(1e-40)
    assert 0 < tiny < np.finfo(np.float32).tiny
    for sval in (F32(np.inf), F32(np.nan), tiny):
        g = base_g.copy()
        g[17, 100] = sval
        for T in (K, K + 2):
            assert same_grid(run_source(comm1, base_a, g, T), np_run(base_a, g, T)), (K, sval, T)
    # grid values outside the range of the plain sweep's scaled walk, and a subnormal grid
    for aval in (F32(1e35), F32(1e-36), tiny):
        a = base_a.copy()
        a[20, 100] = a[5, 240] = aval
        assert same_grid(run_source(comm1, a, base_g, K), np_run(a, base_g, K)), (K, aval)
    a = (base_a.astype(np.float64) * 1e-40).astype(np.float32)
    g = (base_g.astype(np.float64) * 1e-41).astype(np.float32)
    want = np_run(a, g, K)
    assert 0 < np.abs(want[1:-1, 1:-1]).max() < np.finfo(np.float32).tiny
    assert np.array_equal(bits(run_source(comm1, a, g, K)), bits(want))


# ------------------------------------------------------------ 8. decomposed --
def decomposed_run(grid, g, PX, PY, overlap, T):
    from smi_amd import LocalGroup, stencil
    stencil.set_tuning(overlap=overlap)
    tiles, srcs = stencil.split_memory(grid, PX, PY), stencil.split_memory(g, PX, PY)

    def rank_fn(comm):
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            t = torch.from_numpy(tiles[comm.rank]).cuda()
            src = torch.from_numpy(srcs[comm.rank]).cuda()
            res = stencil.run(comm, t, T, PX, PY, source=src)
            s.synchronize()
            return res.cpu().numpy()

    try:
        out = LocalGroup(PX * PY).run(rank_fn)
    finally:
        stencil.set_tuning(overlap=1)
    return stencil.combine_memory(out, PX, PY)


@pytest.mark.parametrize("overlap", [0, 1])
@pytest.mark.parametrize("fuse", [1, 5])
@pytest.mark.parametrize("pxpy", [(2, 1), (1, 2), (2, 2), (3, 3)])
def test_decomposed_run(gpu, restore_settings, pxpy, fuse, overlap):
    """32x64 tiles, T = 7: single steps on every rank whatever the fusion setting."""
    from smi_amd import stencil
    PX, PY = pxpy
    stencil.set_fusion(steps_per_pass=fuse, rows_per_wave=-1)
    assert stencil.plan(32, 64, PX, PY, 0, 7, source=True)["phases"] == [(1, 7)]
    shape = (32 * PX, 64 * PY)
    a, g = uniform(shape, PX * 10 + PY), uniform(shape, PX + 10 * PY)
    got = decomposed_run(a, g, PX, PY, overlap, 7)
    assert np.array_equal(bits(got), bits(np_run(a, g, 7))), (pxpy, fuse, overlap)


# ----------------------------------------------------------------- 9. solve --
@pytest.fixture(scope="module")
def solve_case(oracle_mod):
    """64x96, init_edges, source 0.01 uniform (seed 3), tol 1e-3, check every 8:
    the numpy loop with the same check points."""
    a = oracle_mod.init_edges(64, 96)
    g = (F32(0.01) * oracle_mod.init_uniform(64, 96, seed=3)).astype(np.float32)
    tol, ce, max_steps = 1e-3, 8, 4000
    x, done, r = a, 0, F32(np.inf)
    while done < max_steps:
        prev = np_run(x, g, ce - 1)
        x = np_step(prev, g)
        done += ce
        r = np_resid(x, prev)
        if r <= F32(tol):
            break
    assert 8 < done < max_steps and r <= F32(tol)
    return a, g, tol, ce, max_steps, done, r, x


def test_solve_source_single_tile(gpu, comm1, restore_settings, KS, solve_case):
    from smi_amd import stencil
    a, g, tol, ce, max_steps, steps_w, r_w, x_w = solve_case
    src = torch.from_numpy(g).cuda()
    for fuse in (1, KS, 20):
        stencil.set_fusion(steps_per_pass=fuse, rows_per_wave=-1)
        t = torch.from_numpy(a.copy()).cuda()
        res, steps, r, conv = stencil.solve(comm1, t, tol, max_steps, ce, 1, 1, source=src)
        torch.cuda.synchronize()
        print("fuse", fuse, "steps", steps, "want", steps_w, "residual", r, "want", r_w)
        assert steps == steps_w and conv and same_f32(r, r_w), (fuse, steps, r)
        assert np.array_equal(bits(res.cpu().numpy()), bits(x_w)), fuse
    # max_steps below convergence
    short = steps_w - 2 * ce - 3
    prev = np_run(a, g, short - 1)
    want = np_step(prev, g)
    t = torch.from_numpy(a.copy()).cuda()
    res, steps, r, conv = stencil.solve(comm1, t, tol, short, ce, 1, 1, source=src)
    torch.cuda.synchronize()
    assert np_resid(want, prev) > F32(tol)
    assert steps == short and not conv and same_f32(r, np_resid(want, prev))
    assert np.array_equal(bits(res.cpu().numpy()), bits(want))


def test_solve_source_2x2(gpu, restore_settings, solve_case):
    from smi_amd import LocalGroup, stencil
    a, g, tol, ce, max_steps, steps_w, r_w, x_w = solve_case
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
        assert steps == steps_w and conv and same_f32(r, r_w), (steps, r)
    assert np.array_equal(bits(stencil.combine_memory([o[0] for o in out], 2, 2)), bits(x_w))


# ----------------------------------------------------------------- 10. plan --
@pytest.mark.parametrize("fuse,T", [(1, 5), (3, 7), (20, 20), (20, 41), (2, 4)])
def test_plan_names_the_result_tensor(gpu, comm1, restore_settings, fuse, T):
    from smi_amd import stencil
    stencil.set_fusion(steps_per_pass=fuse, rows_per_wave=-1)
    st, g = states_of((40, 260))
    p = stencil.plan(40, 260, 1, 1, 0, T, source=True)
    t = torch.from_numpy(st[0].copy()).cuda()
    scratch = torch.empty_like(t)
    res = stencil.run(comm1, t, T, 1, 1, scratch=scratch, source=torch.from_numpy(g.copy()).cuda())
    torch.cuda.synchronize()
    assert res is (t, scratch)[p["result_index"]]
    assert p["result_index"] == sum(n for _, n in p["phases"]) % 2
    if T <= 23:
        assert np.array_equal(bits(res.cpu().numpy()), bits(st[T]))
