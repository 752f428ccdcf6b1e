"""The source-term entry points on the host, no GPU needed: the symbols are
declared, exported and bound, the schedule of a source run is the one the
header states, and a bad source array is refused before any device is touched."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("smi_stencil_step_source", "smi_stencil_run_source", "smi_stencil_solve_source", "smi_stencil_plan_source",
       "smi_stencil_source_max_depth")
SMI_ERR_INVALID_ARG, SMI_ERR_BAD_COMM = -1, -5   # include/smi/status.h


@pytest.fixture(scope="module")
def lib():
    from smi_amd import _lib
    return _lib.load()


@pytest.fixture
def restore_settings(lib):
    from smi_amd import stencil
    fuse = stencil.get_fusion()["steps_per_pass"]
    yield
    stencil.set_fusion(steps_per_pass=fuse)


def test_symbols_declared_exported_bound(lib):
    from smi_amd import _lib, stencil
    header = open(os.path.join(ROOT, "include", "smi", "stencil.h")).read()
    assert "-0" in header and "+0" in header        # both facts about a zero source are in the header comment
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW:
        assert re.search(rf"\bint\s+{name}\s*\(", header), name
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES["smi_stencil_step_source"][1]) == 11
    assert len(_lib.SIGNATURES["smi_stencil_run_source"][1]) == 11
    assert len(_lib.SIGNATURES["smi_stencil_solve_source"][1]) == 16
    assert len(_lib.SIGNATURES["smi_stencil_plan_source"][1]) == len(_lib.SIGNATURES["smi_stencil_plan"][1])
    for fn in (stencil.step, stencil.run, stencil.solve, stencil.plan):
        assert "source" in inspect.signature(fn).parameters
    assert callable(stencil.source_max_depth)


def test_source_max_depth(lib):
    from smi_amd import stencil
    assert 6 <= stencil.source_max_depth() <= 12
    assert lib.smi_stencil_source_max_depth(None) == SMI_ERR_INVALID_ARG


def test_plan_source_single_tile(lib, restore_settings):
    """Fusion 1, 2, 3, KS and 20 with T = KS, KS + 1, 2 KS + 2 and 41: no phase
    of 2 steps or of more than KS, the phases sum to T, passes balanced to
    within one step, a remainder of 1 or 2 as single steps."""
    from smi_amd import stencil
    KS = stencil.source_max_depth()
    for fuse in (1, 2, 3, KS, 20):
        stencil.set_fusion(steps_per_pass=fuse)
        K = min(fuse, KS)
        for T in (KS, KS + 1, 2 * KS + 2, 41):
            p = stencil.plan(96, 128, 1, 1, 0, T, source=True)
            ph = p["phases"]
            assert all(s != 2 and 1 <= s <= KS and n >= 1 for s, n in ph), (fuse, T, ph)
            assert sum(s * n for s, n in ph) == T, (fuse, T, ph)
            assert p["result_index"] == sum(n for _, n in ph) % 2
            assert p["neighbours"] == [-1] * 8
            if K < 3:
                assert ph == [(1, T)]
                continue
            fused = [(s, n) for s, n in ph if s >= 3]
            singles = sum(n for s, n in ph if s == 1)
            if T % K in (1, 2):
                assert fused == [(K, T // K)] and singles == T % K, (fuse, T, ph)
            else:
                # as few passes as K allows, depths within one step of each other, none left over
                assert singles == 0 and sum(n for _, n in fused) == -(-T // K), (fuse, T, ph)
                assert max(s for s, _ in fused) - min(s for s, _ in fused) <= 1, (fuse, T, ph)
    stencil.set_fusion(steps_per_pass=20)
    assert stencil.plan(96, 128, 1, 1, 0, KS, source=True)["phases"] == [(KS, 1)]
    assert stencil.plan(96, 128, 1, 1, 0, KS + 1, source=True)["phases"] == [(KS, 1), (1, 1)]
    assert stencil.plan(96, 128, 1, 1, 0, 0, source=True)["phases"] == []
    # a tile narrower than 8 columns runs single steps
    assert stencil.plan(96, 4, 1, 1, 0, 7, source=True)["phases"] == [(1, 7)]


def test_plan_source_multi_rank_is_single_steps(lib, restore_settings):
    from smi_amd import stencil
    for fuse in (1, 5, 20):
        stencil.set_fusion(steps_per_pass=fuse)
        for rank in range(4):
            for T in (7, 12):
                p = stencil.plan(32, 64, 2, 2, rank, T, source=True)
                assert p["phases"] == [(1, T)]
                assert p["result_index"] == T % 2
                assert p["neighbours"] == stencil.plan(32, 64, 2, 2, rank, T)["neighbours"]


def test_bad_source_is_refused_before_any_device(lib):
    from smi_amd import _lib
    buf = (ctypes.c_float * 256)()
    b0 = (ctypes.addressof(buf) + 15) // 16 * 16
    b1, src = b0 + 32 * 4, b0 + 64 * 4           # three 2 x 4 tiles, apart
    idx, steps, conv = ctypes.c_int(-7), ctypes.c_int(-7), ctypes.c_int(-7)
    res = ctypes.c_float(-7)
    bogus = _lib.SMI_Comm(0, 1, 987654)
    mode = (ctypes.c_int * 4)(0, 0, 0, 0)
    halo = (ctypes.c_void_p * 4)()

    def run(s):
        return lib.smi_stencil_run_source(bogus, b0, b1, s, 2, 4, 1, 1, 5, None, ctypes.byref(idx))

    def solve(s):
        return lib.smi_stencil_solve_source(bogus, b0, b1, s, 2, 4, 1, 1, ctypes.c_float(1e-3), 10, 2, None,
                                            ctypes.byref(idx), ctypes.byref(steps), ctypes.byref(res),
                                            ctypes.byref(conv))

    def step(s):
        return lib.smi_stencil_step_source(b0, b1, s, 2, 4, mode, halo, None, None, None, None)

    for call in (run, solve, step):
        for bad, what in ((None, "NULL"), (src + 4, "aligned"), (b0, "overlap"), (b1 + 16, "overlap")):
            assert call(bad) == SMI_ERR_INVALID_ARG, (call.__name__, what)
            assert what in lib.smi_last_error().decode(), (call.__name__, what, lib.smi_last_error())
    # a good source passes that check: the run and the solve then miss their communicator
    assert run(src) == SMI_ERR_BAD_COMM and solve(src) == SMI_ERR_BAD_COMM
    assert idx.value == -7 and steps.value == -7
    # the plain counterparts answer a bad buffer the same way
    assert lib.smi_stencil_step(None, b1, 2, 4, mode, halo, None, None, None) == SMI_ERR_INVALID_ARG
