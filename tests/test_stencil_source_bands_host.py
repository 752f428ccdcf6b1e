"""smi_stencil_set_source_bands on the host, no GPU needed: the switch itself and
the schedule of a multi-rank source run under both settings (the rules of
include/smi/stencil.h: K = min(steps_per_pass, KS) clipped to a tile of 2K rows
and 8 ceil(K/4) columns, the balanced-remainder rule, a remainder of 1 or 2 as
single steps)."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMI_ERR_INVALID_ARG = -1   # include/smi/status.h


@pytest.fixture(scope="module")
def lib():
    from smi_amd import _lib
    return _lib.load()


@pytest.fixture
def restore_settings(lib):
    from smi_amd import stencil
    fuse, bands = stencil.get_fusion()["steps_per_pass"], stencil.get_source_bands()
    yield
    stencil.set_fusion(steps_per_pass=fuse)
    stencil.set_source_bands(bands)


def phases(x, y, px, py, rank, T):
    from smi_amd import stencil
    return stencil.plan(x, y, px, py, rank, T, source=True)["phases"]


def test_symbols_declared_exported_bound(lib):
    from smi_amd import _lib, stencil
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "smi", "stencil.h")).read(), flags=re.S)
    for name in ("smi_stencil_set_source_bands", "smi_stencil_get_source_bands"):
        assert re.search(rf"\bint\s+{name}\s*\(", header), name
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert callable(stencil.set_source_bands) and callable(stencil.get_source_bands)


def test_switch_default_round_trip_and_keep(lib, restore_settings):
    from smi_amd import stencil
    assert stencil.get_source_bands() == 0                     # the default (every test restores it)
    stencil.set_source_bands(1)
    assert stencil.get_source_bands() == 1
    stencil.set_source_bands(-1)
    assert stencil.get_source_bands() == 1                     # -1 keeps the setting
    stencil.set_source_bands()
    assert stencil.get_source_bands() == 1
    stencil.set_source_bands(0)
    assert stencil.get_source_bands() == 0
    stencil.set_source_bands(-1)
    assert stencil.get_source_bands() == 0
    assert lib.smi_stencil_set_source_bands(2) == SMI_ERR_INVALID_ARG
    assert stencil.get_source_bands() == 0
    assert lib.smi_stencil_get_source_bands(None) == 0         # a NULL output is allowed, like the other getters


def test_switch_off_multi_rank_plans_are_single_steps(lib, restore_settings):
    from smi_amd import stencil
    stencil.set_source_bands(0)
    for fuse in (1, 5, 20):
        stencil.set_fusion(steps_per_pass=fuse)
        for shape in ((72, 136), (32, 64), (10, 16)):
            for rank in range(4):
                for T in (7, 13):
                    assert phases(*shape, 2, 2, rank, T) == [(1, T)], (fuse, shape, rank, T)


def test_switch_on_the_stated_plans(lib, restore_settings):
    from smi_amd import stencil
    KS = stencil.source_max_depth()
    stencil.set_source_bands(1)
    stencil.set_fusion(steps_per_pass=5)
    for rank in range(4):
        assert phases(72, 136, 2, 2, rank, 13) == [(5, 1), (4, 2)]
        assert phases(72, 136, 2, 2, rank, 7) == [(5, 1), (1, 2)]
    # fusion 20 plans K = KS
    stencil.set_fusion(steps_per_pass=20)
    assert phases(72, 136, 2, 2, 0, KS) == [(KS, 1)]
    assert phases(72, 136, 2, 2, 0, 3 * KS) == [(KS, 3)]
    assert phases(72, 136, 2, 2, 0, KS + 1) == [(KS, 1), (1, 1)]
    # a 10 x 16 tile holds 2K rows for K <= 5 and 8 ceil(K/4) columns for K <= 8
    assert phases(10, 16, 2, 2, 0, 5) == [(5, 1)]
    assert phases(10, 16, 2, 2, 0, 10) == [(5, 2)]
    assert phases(10, 16, 2, 2, 0, 9) == [(5, 1), (4, 1)]
    # too small for any K-step pass: single steps
    assert phases(4, 8, 2, 2, 0, 7) == [(1, 7)]
    assert phases(72, 4, 2, 2, 0, 7) == [(1, 7)]
    # a fusion setting below 3: single steps
    for fuse in (1, 2):
        stencil.set_fusion(steps_per_pass=fuse)
        assert phases(72, 136, 2, 2, 0, 7) == [(1, 7)]


def test_switch_on_every_plan_keeps_the_rules(lib, restore_settings):
    """No phase of depth 2 or > KS, at most 2 phases, the steps sum to T, the
    result index is the pass count mod 2, the same schedule on every rank."""
    from smi_amd import stencil
    KS = stencil.source_max_depth()
    stencil.set_source_bands(1)
    for fuse in (1, 2, 3, 5, KS, 12, 20):
        stencil.set_fusion(steps_per_pass=fuse)
        for shape, grid in (((72, 136), (2, 2)), ((61, 140), (3, 3)), ((10, 16), (2, 3)), ((16, 24), (1, 2))):
            X, Y = shape
            kt = min(fuse, KS, X // 2, max(k for k in range(0, 21) if 8 * ((k + 3) // 4) <= Y))
            for T in (0, 1, 2, 3, 7, KS, KS + 1, 2 * KS + 1, 2 * KS + 5, 41):
                plans = [stencil.plan(X, Y, *grid, r, T, source=True) for r in range(grid[0] * grid[1])]
                ph = plans[0]["phases"]
                assert all(p["phases"] == ph for p in plans), (fuse, shape, T)
                assert len(ph) <= 2, (fuse, shape, T, ph)
                assert all(s != 2 and 1 <= s <= KS and n >= 1 for s, n in ph), (fuse, shape, T, ph)
                assert sum(s * n for s, n in ph) == T, (fuse, shape, T, ph)
                assert all(p["result_index"] == sum(n for _, n in ph) % 2 for p in plans)
                if kt < 3:
                    assert ph == ([(1, T)] if T else []), (fuse, shape, T, ph)
                    continue
                fused = [(s, n) for s, n in ph if s >= 3]
                singles = sum(n for s, n in ph if s == 1)
                assert all(s <= kt for s, _ in fused), (fuse, shape, T, ph)
                if T % kt in (1, 2):
                    assert fused == ([(kt, T // kt)] if T >= kt else []) and singles == T % kt, (fuse, shape, T, ph)
                else:
                    assert singles == 0 and sum(n for _, n in fused) == -(-T // kt), (fuse, shape, T, ph)
                    assert not fused or max(s for s, _ in fused) - min(s for s, _ in fused) <= 1


def test_single_tile_plans_do_not_depend_on_the_switch(lib, restore_settings):
    from smi_amd import stencil
    KS = stencil.source_max_depth()
    for fuse in (1, 3, KS, 20):
        stencil.set_fusion(steps_per_pass=fuse)
        for shape in ((96, 128), (10, 16), (4, 8), (96, 4)):
            for T in (0, 2, 7, KS + 1, 2 * KS + 5):
                stencil.set_source_bands(0)
                off = stencil.plan(*shape, 1, 1, 0, T, source=True)
                stencil.set_source_bands(1)
                assert stencil.plan(*shape, 1, 1, 0, T, source=True) == off, (fuse, shape, T)
    # and the plain and the residual schedules of a multi-rank run ignore it
    stencil.set_fusion(steps_per_pass=5)
    for kw in ({}, {"residual": True}):
        stencil.set_source_bands(0)
        off = stencil.plan(72, 136, 2, 2, 0, 13, **kw)
        stencil.set_source_bands(1)
        assert stencil.plan(72, 136, 2, 2, 0, 13, **kw) == off
