"""smi_stencil_run_residual on the GPU: a run whose last K-step pass also
returns max |x_T - x_{T-1}| of this rank's tile, and smi_stencil_solve with the
fused check (smi_stencil_set_solve_check(1)).

Every comparison is bit for bit, against the CPU oracle's states x_{T-1} and
x_T and numpy's max(abs(x_T - x_{T-1})) -- the np_resid contract of
tests/test_stencil_solve_gpu.py (one fp32 subtraction and fabs per cell, NaN if
any difference is NaN).  Nothing is compared with the library's own output.
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


def same_grid(got, want):
    """bit-identical, all NaNs equal"""
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got)[~nan], bits(want)[~nan])


@pytest.fixture
def restore_settings(gpu):
    from smi_amd import stencil
    tune, fuse, check = stencil.get_tuning(), stencil.get_fusion()["steps_per_pass"], stencil.get_solve_check()
    stencil.set_fusion(steps_per_pass=12)
    htk = stencil.get_fusion()["rows_per_wave"]          # the K-step sweep's rows per wave (0: automatic)
    stencil.set_fusion(steps_per_pass=fuse)
    yield
    stencil.set_tuning(tune["rows_per_wave"], tune["rows_in_flight"], tune["nontemporal"], tune["overlap"])
    stencil.set_fusion(steps_per_pass=12, rows_per_wave=htk if htk > 0 else -1)
    stencil.set_fusion(steps_per_pass=fuse)
    stencil.set_solve_check(check)


@pytest.fixture(scope="module")
def comm1(gpu):
    from smi_amd import LocalGroup
    comm = LocalGroup(1).comm(0)
    yield comm
    comm.finalize()


def run_residual(comm, grid, T, word=None):
    """(grid after T steps, residual word) of run(..., residual=word) on one tile."""
    from smi_amd import stencil
    t = torch.from_numpy(np.array(grid, dtype=np.float32)).cuda()      # (a writable copy: the shared states are not)
    if word is None:
        word = torch.zeros(1, dtype=torch.int32, device="cuda")
    res = stencil.run(comm, t, T, 1, 1, residual=word)
    torch.cuda.synchronize()
    return res.cpu().numpy(), word


def last_two(oracle_mod, g, T):
    """the oracle's x_{T-1} and x_T"""
    prev = oracle_mod.stencil(g, T - 1) if T > 1 else np.ascontiguousarray(g, dtype=np.float32)
    return prev, oracle_mod.stencil(prev, 1)


def k_of(fuse):
    return min(fuse, 12)


# the sweep's window geometry (smi_amd/csrc/stencilk.h): apron lanes per side,
# output columns per 256-column window
def window_cols(K):
    return 256 - 8 * (4 if K >= 9 else (K + 3) // 4)


# ------------------------------------------------------------- one tile --
SHAPES = [(26, 8), (40, 260), (40, 300), (129, 516)]
_STATES = {}


def states_of(oracle_mod, shape, init):
    """oracle states x_0..x_41 of a start grid, computed once per module"""
    key = (shape, init)
    if key not in _STATES:
        X, Y = shape
        g = oracle_mod.init_edges(X, Y) if init == "edges" else oracle_mod.init_uniform(X, Y, seed=X * 31 + Y)
        st = [g]
        for _ in range(41):
            st.append(oracle_mod.stencil(st[-1], 1))
        for s in st:
            s.setflags(write=False)
        _STATES[key] = st
    return _STATES[key]


@pytest.mark.parametrize("init", ["edges", "uniform"])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("fuse", [3, 4, 7, 12, 20])
def test_grid_and_residual_one_tile(gpu, oracle_mod, comm1, restore_settings, fuse, shape, init):
    """steps_per_pass 3, 4, 7, 12 and 20 (K_r = 12); T = K, K + 1, 2K + 5 and
    41; rows per wave automatic and 40 (129 rows: 4 row blocks)."""
    from smi_amd import stencil
    K = k_of(fuse)
    st = states_of(oracle_mod, shape, init)
    for rpw in (-1, 40):
        stencil.set_fusion(steps_per_pass=fuse, rows_per_wave=rpw)
        for T in sorted({K, K + 1, 2 * K + 5, 41}):
            want_r = np_resid(st[T], st[T - 1])
            got, word = run_residual(comm1, st[0], T)
            got_r = word_value(word)
            print(fuse, shape, init, rpw, T, "residual", got_r, "want", want_r)
            assert np.array_equal(bits(got), bits(st[T])), (fuse, shape, rpw, T)
            assert same_f32(got_r, want_r), (fuse, shape, rpw, T, got_r, want_r)


@pytest.mark.parametrize("fuse,T", [(1, 5), (2, 5), (20, 1), (20, 2), (12, 2)])
def test_runs_that_end_in_a_single_residual_step(gpu, oracle_mod, comm1, restore_settings, fuse, T):
    """A fusion setting of 1 or 2 and runs of fewer than 3 steps: the last
    launch is one single residual step (K_r < 3)."""
    from smi_amd import stencil
    stencil.set_fusion(steps_per_pass=fuse)
    assert stencil.plan(40, 260, 1, 1, 0, T, residual=True)["phases"][-1] == (1, 1)
    st = states_of(oracle_mod, (40, 260), "uniform")
    got, word = run_residual(comm1, st[0], T)
    assert np.array_equal(bits(got), bits(st[T]))
    assert same_f32(word_value(word), np_resid(st[T], st[T - 1]))


# -------------------------------------------------------- single spikes --
def spike_grid(shape, target, T, value=F32(3.0e6)):
    """Zeros plus one large cell such that the largest |x_T - x_{T-1}| sits at
    `target`: x_{T-1} peaks at the spike itself when T - 1 is even; when it is
    odd the spike's four neighbours tie, so two spikes go left and right of the
    target, which then collects both peaks."""
    g = np.zeros(shape, dtype=np.float32)
    r, c = target
    if (T - 1) % 2 == 0:
        g[r, c] = value
    else:
        g[r, c - 1] = value
        g[r, c + 1] = value
    return g


def _spike_cases():
    """(name, shape, rows per wave, K, cell the spike aims at, region) --
    region = (row range, column range) the oracle's argmax must lie in."""
    cases = []
    for K in (3, 12):
        sw = window_cols(K)
        # both columns at a strip boundary of a 516-wide tile
        cases.append((f"strip_last_col_K{K}", (40, 516), -1, K, (20, sw - 1), ((0, 40), (sw - 1, sw))))
        cases.append((f"strip_first_col_K{K}", (40, 516), -1, K, (20, sw), ((0, 40), (sw, sw + 1))))
        # first and last stored lane of the second window (4 columns each)
        cases.append((f"first_stored_lane_K{K}", (40, 516), -1, K, (9, sw + 2), ((0, 40), (sw, sw + 4))))
        cases.append((f"last_stored_lane_K{K}", (40, 516), -1, K, (9, 2 * sw - 3), ((0, 40), (2 * sw - 4, 2 * sw))))
        # the last, partial strip of a 300-wide tile
        cases.append((f"partial_strip_K{K}", (40, 300), -1, K, (30, 290), ((0, 40), (sw, 300))))
        cases.append((f"partial_strip_end_K{K}", (40, 300), -1, K, (11, 297), ((0, 40), (296, 300))))
        # both rows at a row-block boundary: 129 rows, 40 per wave -> blocks start at 0, 32, 64, 96
        cases.append((f"block_last_row_K{K}", (129, 516), 40, K, (63, 100), ((63, 64), (0, 516))))
        cases.append((f"block_first_row_K{K}", (129, 516), 40, K, (64, 300), ((64, 65), (0, 516))))
        # rows and columns next to each global edge.  The copied edge (zeros) absorbs: after 3
        # steps the peak is still in the line next to it, after 12 it has moved up to two lines
        # further in, so K = 12 names the three lines beside the edge.
        n = 1 if K == 3 else 3
        cases.append((f"next_to_top_K{K}", (40, 260), -1, K, (1, 130), ((1, 1 + n), (0, 260))))
        cases.append((f"next_to_bottom_K{K}", (40, 260), -1, K, (38, 131), ((39 - n, 39), (0, 260))))
        cases.append((f"next_to_left_K{K}", (40, 260), -1, K, (20, 1), ((0, 40), (1, 1 + n))))
        cases.append((f"next_to_right_K{K}", (40, 260), -1, K, (21, 258), ((0, 40), (259 - n, 259))))
    return cases


@pytest.mark.parametrize("name,shape,rpw,K,target,region", _spike_cases(), ids=[c[0] for c in _spike_cases()])
def test_single_spike_argmax_is_counted(gpu, oracle_mod, comm1, restore_settings, name, shape, rpw, K, target,
                                        region):
    """T = K_r = 3 and 12 on zeros plus a spike: the oracle's largest final
    difference is unique and lies in the named region, so a cell of that
    region left out of the maximum gives a smaller word."""
    from smi_amd import stencil
    T = K
    if name.startswith("next_to_left") or name.startswith("next_to_right"):
        # the pair of spikes goes above and below the target here (column 0 / Y-1 is the copied edge)
        g = spike_grid(shape[::-1], target[::-1], T).T.copy()
    else:
        g = spike_grid(shape, target, T)
    prev, want = last_two(oracle_mod, g, T)
    d = np.abs(want - prev)
    where = np.unravel_index(np.argmax(d), d.shape)
    (r0, r1), (c0, c1) = region
    assert r0 <= where[0] < r1 and c0 <= where[1] < c1, (name, where)
    assert (d == d.max()).sum() == 1        # unique: no other cell can stand in for it
    stencil.set_fusion(steps_per_pass=K, rows_per_wave=rpw)
    got, word = run_residual(comm1, g, T)
    assert np.array_equal(bits(got), bits(want)), name
    assert same_f32(word_value(word), np_resid(want, prev)), (name, word_value(word), d.max())


@pytest.mark.parametrize("K", [3, 12])
@pytest.mark.parametrize("cell", [(0, 5), (39, 131), (20, 0), (7, 259)])
def test_spike_in_a_global_edge_cell(gpu, oracle_mod, comm1, restore_settings, K, cell):
    """A copied edge cell contributes |c - c| = 0 whatever it holds; the
    largest difference is in the line next to it.  With +inf in the edge cell
    |c - c| is inf - inf: the residual is NaN, as numpy says."""
    from smi_amd import stencil
    stencil.set_fusion(steps_per_pass=K, rows_per_wave=-1)
    g = np.zeros((40, 260), dtype=np.float32)
    g[cell] = F32(3.0e6)
    prev, want = last_two(oracle_mod, g, K)
    d = np.abs(want - prev)
    where = np.unravel_index(np.argmax(d), d.shape)
    assert d[cell] == 0 and d.max() > 1
    inner = (min(max(cell[0], 1), 38), min(max(cell[1], 1), 258))
    assert abs(where[0] - inner[0]) + abs(where[1] - inner[1]) <= K        # beside the edge cell, not on it
    got, word = run_residual(comm1, g, K)
    assert np.array_equal(bits(got), bits(want))
    assert same_f32(word_value(word), np_resid(want, prev))
    g[cell] = np.inf
    prev, want = last_two(oracle_mod, g, K)
    assert np.isnan(np_resid(want, prev))
    got, word = run_residual(comm1, g, K)
    assert same_grid(got, want)
    assert np.isnan(word_value(word))


# ------------------------------------------- unstored lanes must not count --
@pytest.mark.parametrize("K", [3, 7, 12])
def test_apron_lanes_and_rows_outside_the_block_do_not_count(gpu, oracle_mod, comm1, restore_settings, K):
    """Guards against a register maximum that forgets the store's mask.  The
    grid is a steep plane 1000 + 3 i + 5 j plus noise of 1e-3: a plane is a
    fixed point of the Jacobi step (copied edges included), so the true final
    difference is of the order of the noise.  The values the kernel holds
    where it does NOT store are far rougher than that: the outermost lanes of
    a 256-column window take a W / E neighbour of 0 from the lane shift (an
    error of ~250 per level that spreads through the apron lanes), and input
    rows past the tile's end are clamped copies (a jump of 3 per row) that
    feed the rows a block computes outside [o0, o1).  Were any apron lane, any
    row outside its block or any column outside [col_lo, col_hi) counted, the
    word would be ~1e2 instead of ~1e-3.  516 columns: three windows; 129 rows
    at 40 rows per wave: four row blocks."""
    from smi_amd import stencil
    X, Y = 129, 516
    i, j = np.indices((X, Y))
    rng = np.random.default_rng(K)
    g = (1000.0 + 3.0 * i + 5.0 * j + 1e-3 * rng.random((X, Y))).astype(np.float32)
    for T in (K, 2 * K + 5):
        prev, want = last_two(oracle_mod, g, T)
        want_r = np_resid(want, prev)
        assert 0 < want_r < 0.01
        for rpw in (-1, 40):
            stencil.set_fusion(steps_per_pass=K, rows_per_wave=rpw)
            got, word = run_residual(comm1, g, T)
            print(K, T, rpw, "residual", word_value(word), "want", want_r)
            assert np.array_equal(bits(got), bits(want))
            assert same_f32(word_value(word), want_r), (K, T, rpw, word_value(word), want_r)


# --------------------------------------------------------- guard fallback --
@pytest.mark.parametrize("cell_value", [1e35, 1e-36])
@pytest.mark.parametrize("pos", [(20, 100), (5, 240)])
def test_guard_fallback_discards_the_scaled_walk(gpu, oracle_mod, comm1, restore_settings, cell_value, pos):
    """One cell outside [2^-100, 2^101) in an ordinary (40, 260) grid, K = 12:
    the waves that read it fail the scaled walk's guard and walk again with the
    exact arithmetic; the scaled walk's maximum (1e35 x 4^11 overflows there: an
    inf or NaN) must not survive."""
    from smi_amd import stencil
    stencil.set_fusion(steps_per_pass=12, rows_per_wave=-1)
    g = oracle_mod.init_uniform(40, 260, seed=12).copy()
    g[pos] = F32(cell_value)
    prev, want = last_two(oracle_mod, g, 12)
    want_r = np_resid(want, prev)
    assert np.isfinite(want_r) and want_r > 0
    got, word = run_residual(comm1, g, 12)
    assert np.array_equal(bits(got), bits(want))
    assert np.isfinite(word_value(word))
    assert same_f32(word_value(word), want_r), (word_value(word), want_r)


# ---------------------------------------------------------- special values --
@pytest.mark.parametrize("K", [3, 12])
def test_nan_negative_zero_and_subnormals(gpu, oracle_mod, comm1, restore_settings, K):
    from smi_amd import stencil
    stencil.set_fusion(steps_per_pass=K, rows_per_wave=-1)
    # one NaN cell: a NaN residual
    g = oracle_mod.init_uniform(40, 264, seed=6).copy()
    g[17, 100] = np.nan
    prev, want = last_two(oracle_mod, g, K)
    got, word = run_residual(comm1, g, K)
    assert same_grid(got, want)
    assert np.isnan(np_resid(want, prev)) and np.isnan(word_value(word))
    # +0 cells among -0 neighbours: differences of -0, whose sign fabs clears
    i, j = np.indices((24, 264))
    g = np.where((i + j) % 2 == 0, F32(0.0), F32(-0.0)).astype(np.float32)
    prev, want = last_two(oracle_mod, g, K)
    if K == 3:
        assert np.signbit(want - prev).any()       # (after 12 steps every sum has met a +0)
    got, word = run_residual(comm1, g, K)
    assert np.array_equal(bits(got), bits(want))
    assert int(word.cpu().numpy()[0]) == 0
    # a grid in the subnormal range keeps its (subnormal) differences
    g = (oracle_mod.init_uniform(40, 264, seed=4).astype(np.float64) * 1e-40).astype(np.float32)
    prev, want = last_two(oracle_mod, g, K)
    want_r = np_resid(want, prev)
    assert 0 < want_r < np.finfo(np.float32).tiny
    got, word = run_residual(comm1, g, K)
    assert np.array_equal(bits(got), bits(want))
    assert same_f32(word_value(word), want_r), (word_value(word), want_r)


def test_inf_cell_in_the_interior(gpu, oracle_mod, comm1, restore_settings):
    """inf spreads one cell per step with alternating parity: x_T and x_{T-1}
    are never both inf in one cell, the residual is +inf; two inf cells at an
    odd distance meet: inf - inf = NaN.  Both as numpy has them."""
    from smi_amd import stencil
    stencil.set_fusion(steps_per_pass=12, rows_per_wave=-1)
    for cells in ([(19, 130)], [(19, 100), (19, 103)]):
        g = oracle_mod.init_uniform(40, 264, seed=7).copy()
        for rc in cells:
            g[rc] = np.inf
        prev, want = last_two(oracle_mod, g, 12)
        want_r = np_resid(want, prev)
        assert np.isposinf(want_r) if len(cells) == 1 else np.isnan(want_r)
        got, word = run_residual(comm1, g, 12)
        assert same_grid(got, want)
        assert same_f32(word_value(word), want_r), (cells, word_value(word), want_r)


# ------------------------------------------------------------ accumulation --
def test_two_runs_accumulate_into_one_word(gpu, oracle_mod, comm1, restore_settings):
    from smi_amd import stencil
    stencil.set_fusion(steps_per_pass=7, rows_per_wave=-1)
    small = oracle_mod.init_uniform(33, 264, seed=1)
    big = oracle_mod.init_uniform(26, 8, seed=2) * F32(64)
    r_small = np_resid(*last_two(oracle_mod, small, 7)[::-1])
    r_big = np_resid(*last_two(oracle_mod, big, 7)[::-1])
    assert r_big > r_small > 0
    for first, second in ((small, big), (big, small)):
        _, word = run_residual(comm1, first, 7)
        _, word = run_residual(comm1, second, 7, word=word)      # not zeroed in between
        assert same_f32(word_value(word), r_big)
    word = torch.from_numpy(np.array([1e9], dtype=np.float32).view(np.int32)).cuda()
    _, word = run_residual(comm1, big, 7, word=word)
    assert same_f32(word_value(word), F32(1e9))


# -------------------------------------------------------------- decomposed --
def decomposed_run(grid, PX, PY, overlap, T):
    """(combined grid, per-rank residual values) of run(..., residual=word) on every rank, in process."""
    from smi_amd import LocalGroup, stencil
    stencil.set_tuning(overlap=overlap)
    tiles = stencil.split_memory(grid, PX, PY)

    def rank_fn(comm):
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            t = torch.from_numpy(tiles[comm.rank]).cuda()
            word = torch.zeros(1, dtype=torch.int32, device="cuda")
            res = stencil.run(comm, t, T, PX, PY, residual=word)
            s.synchronize()
            return res.cpu().numpy(), word_value(word)

    try:
        out = LocalGroup(PX * PY).run(rank_fn)
    finally:
        stencil.set_tuning(overlap=1)
    return stencil.combine_memory([o[0] for o in out], PX, PY), [o[1] for o in out]


def rank_masks(shape, PX, PY):
    X, Y = shape
    XL, YL = X // PX, Y // PY
    masks = []
    for r in range(PX * PY):
        m = np.zeros(shape, dtype=bool)
        m[(r // PY) * XL:(r // PY + 1) * XL, (r % PY) * YL:(r % PY + 1) * YL] = True
        masks.append(m)
    return masks


def check_decomposed(oracle_mod, g, PX, PY, overlap, T):
    prev, want = last_two(oracle_mod, g, T)
    got, words = decomposed_run(g, PX, PY, overlap, T)
    assert np.array_equal(bits(got), bits(want)), (PX, PY, overlap, T)
    for rank, m in enumerate(rank_masks(g.shape, PX, PY)):
        want_r = np_resid(want, prev, m)
        print((PX, PY), overlap, T, "rank", rank, "residual", words[rank], "want", want_r)
        assert same_f32(words[rank], want_r), (PX, PY, overlap, T, rank, words[rank], want_r)


@pytest.mark.parametrize("overlap", [0, 1])
@pytest.mark.parametrize("fuse", [5, 12])
@pytest.mark.parametrize("pxpy", [(2, 1), (1, 2), (2, 2), (3, 3)])
def test_decomposed_grid_and_per_rank_residual(gpu, oracle_mod, restore_settings, pxpy, fuse, overlap):
    """32x64 tiles; T = K_r and 2 K_r + 3; each rank's word is numpy's maximum
    over that rank's tile region (the residual is rank-local)."""
    from smi_amd import stencil
    PX, PY = pxpy
    stencil.set_fusion(steps_per_pass=fuse, rows_per_wave=-1)
    assert stencil.plan(32, 64, PX, PY, 0, 2 * fuse + 3, residual=True)["phases"][-1] == (fuse, 1)
    g = oracle_mod.init_uniform(32 * PX, 64 * PY, seed=PX * 10 + PY)
    for T in (fuse, 2 * fuse + 3):
        check_decomposed(oracle_mod, g, PX, PY, overlap, T)


def _band_targets(K):
    """2x2 of 32x64 tiles; rank 3 (rows 32..63, columns 64..127) has a top and
    a left neighbour.  Its bands are K rows / KC = 4 ceil(K/4) columns deep."""
    kc = 4 * ((K + 3) // 4)
    return [("top_band", (32 + K // 2, 100), ((32, 32 + K), (64, 128))),
            ("left_band", (50, 64 + kc // 2), ((32 + K, 64), (64, 64 + kc))),
            ("corner_block", (33, 66), ((32, 32 + K), (64, 64 + kc))),
            ("interior_row_next_to_band", (32 + K, 101), ((32 + K, 33 + K), (64 + kc, 128))),
            ("interior_col_next_to_band", (51, 64 + kc), ((32 + K, 64), (64 + kc, 65 + kc)))]


@pytest.mark.parametrize("K", [5, 12])
@pytest.mark.parametrize("which", range(5))
def test_decomposed_spike_in_bands_and_beside_them(gpu, oracle_mod, restore_settings, K, which):
    """The oracle's unique largest final difference lies in a band of rank 3,
    in its corner block, or in the interior row / column next to a band: each
    cell is counted by exactly the kernel that stores it."""
    from smi_amd import stencil
    name, target, region = _band_targets(K)[which]
    stencil.set_fusion(steps_per_pass=K, rows_per_wave=-1)
    g = spike_grid((64, 128), target, K)
    prev, want = last_two(oracle_mod, g, K)
    d = np.abs(want - prev)
    where = np.unravel_index(np.argmax(d), d.shape)
    (r0, r1), (c0, c1) = region
    assert where == tuple(target) and r0 <= where[0] < r1 and c0 <= where[1] < c1, (name, where)
    assert (d == d.max()).sum() == 1
    check_decomposed(oracle_mod, g, 2, 2, 1, K)


# ------------------------------------------------- solve, fused check on --
def oracle_sequence(oracle_mod, g, T):
    states, r = [np.ascontiguousarray(g, dtype=np.float32)], [None]
    for _ in range(T):
        nxt = oracle_mod.stencil(states[-1], 1)
        r.append(np_resid(nxt, states[-1]))
        states.append(nxt)
    return states, r


def expected_stop(r, tol, max_steps, check_every):
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


def run_solve(comm, g, tol, max_steps, check_every):
    from smi_amd import stencil
    t = torch.from_numpy(np.ascontiguousarray(g)).cuda()
    res, steps, r, conv = stencil.solve(comm, t, tol, max_steps, check_every, 1, 1)
    torch.cuda.synchronize()
    return res.cpu().numpy(), steps, r, conv


@pytest.mark.parametrize("tol,check_every,max_steps", [
    (1e-3, 1, 600), (1e-3, 7, 600), (1e-3, 20, 600), (1e-3, 64, 600), (0.0, 1, 1500),
    (1e-3, 64, 250), (1e-3, 64, 100), (1e-3, 20, 200)])
def test_solve_single_tile_both_checks(gpu, seq16, comm1, restore_settings, tol, check_every, max_steps):
    from smi_amd import stencil
    states, r = seq16
    steps_w, r_w, conv_w = expected_stop(r, tol, max_steps, check_every)
    for fused in (1, 0):
        stencil.set_solve_check(fused)
        got, steps, res, conv = run_solve(comm1, states[0], tol, max_steps, check_every)
        print("fused", fused, "steps", steps, "want", steps_w, "residual", res, "want", r_w, "converged", conv)
        assert steps == steps_w, fused
        assert same_f32(res, r_w), (fused, res, r_w)
        assert conv == conv_w, fused
        assert np.array_equal(bits(got), bits(states[steps])), fused


def test_solve_is_fusion_neutral_both_checks(gpu, oracle_mod, comm1, restore_settings):
    """96x128, check_every = 41, steps_per_pass 1, 2, 12 and 20: with the fused
    check the 41 steps up to a check point run as 15 + 14 + a 12-step residual
    pass under steps_per_pass = 20."""
    from smi_amd import stencil
    g = oracle_mod.init_uniform(96, 128, seed=96)
    tol, ce, max_steps = 0.07, 41, 200
    r, states, x = {}, {}, g
    done = 0
    while done < max_steps:
        nxt = min(done + ce, max_steps)
        prev = oracle_mod.stencil(x, nxt - done - 1)
        x = oracle_mod.stencil(prev, 1)
        r[nxt], states[nxt] = np_resid(x, prev), x
        done = nxt
    steps_w = next((t for t in sorted(r) if r[t] <= F32(tol)), max_steps)
    assert sorted(r)[0] < steps_w < max_steps
    for k in (1, 2, 12, 20):
        for fused in (1, 0):
            stencil.set_fusion(steps_per_pass=k)
            stencil.set_solve_check(fused)
            got, steps, res, conv = run_solve(comm1, g, tol, max_steps, ce)
            print("K", k, "fused", fused, "steps", steps, "want", steps_w, "residual", res, "want", r[steps_w])
            assert steps == steps_w, (k, fused)
            assert same_f32(res, r[steps_w]), (k, fused, res, r[steps_w])
            assert conv == bool(r[steps_w] <= F32(tol))
            assert np.array_equal(bits(got), bits(states[steps_w])), (k, fused)


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
def test_solve_decomposed_both_checks(gpu, oracle_mod, restore_settings, pxpy, overlap):
    from smi_amd import stencil
    PX, PY = pxpy
    tol, ce, max_steps = 1e-3, 20, 600
    g = stencil.init_grid(16 * PX, 32 * PY)
    states, r = oracle_sequence(oracle_mod, g, max_steps)
    steps_w, r_w, conv_w = expected_stop(r, tol, max_steps, ce)
    for fused in (1, 0):
        stencil.set_solve_check(fused)
        got, per_rank = decomposed_solve(g, PX, PY, overlap, tol, max_steps, ce)
        print(pxpy, overlap, "fused", fused, "want", steps_w, r_w, "got", per_rank)
        for steps, res, conv in per_rank:
            assert steps == steps_w and same_f32(res, r_w) and conv == conv_w, (fused, per_rank, steps_w, r_w)
        assert np.array_equal(bits(got), bits(states[steps_w])), fused


# ---------------------------------------------------- two RCCL processes --
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_solve_fused_check_two_rccl_processes(gpu):
    """tests/solve_fused_worker.py as two fresh child processes, one rank each,
    over the production transport: the cases of tests/solve_worker.py with
    smi_stencil_set_solve_check(1), bit-exact against the oracle.  Each child
    has its own time limit."""
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
        procs.append(subprocess.Popen([sys.executable, "-u", os.path.join(HERE, "solve_fused_worker.py")], env=env,
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
    assert all("SOLVE CHECK FUSED 1" in o for o in outs), log
    assert "SOLVE MULTIPROC PASS" in outs[0], log
    assert sum(o.count(" CASE ") for o in outs) >= 4 and not any("MISMATCH" in o for o in outs), log
