"""smi_stencil_run_residual / smi_stencil_plan_residual / the solve-check
switch on the host, no GPU needed: the symbols are declared, exported and
bound, the schedule of a residual run is the one the header states, and bad
arguments are refused before any device is touched."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("smi_stencil_run_residual", "smi_stencil_plan_residual", "smi_stencil_set_solve_check",
       "smi_stencil_get_solve_check")
SMI_ERR_INVALID_ARG, SMI_ERR_BAD_COMM = -1, -5   # include/smi/status.h


@pytest.fixture(scope="module")
def lib():
    from smi_amd import _lib
    return _lib.load()


@pytest.fixture
def restore_settings(lib):
    from smi_amd import stencil
    fuse, check = stencil.get_fusion()["steps_per_pass"], stencil.get_solve_check()
    yield
    stencil.set_fusion(steps_per_pass=fuse)
    stencil.set_solve_check(check)


def test_symbols_declared_exported_bound(lib):
    import inspect

    from smi_amd import _lib, stencil
    header = open(os.path.join(ROOT, "include", "smi", "stencil.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW:
        assert re.search(rf"\bint\s+{name}\s*\(", header), name
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES["smi_stencil_run_residual"][1]) == 11
    assert len(_lib.SIGNATURES["smi_stencil_plan_residual"][1]) == len(_lib.SIGNATURES["smi_stencil_plan"][1])
    assert "residual" in inspect.signature(stencil.run).parameters
    assert "residual" in inspect.signature(stencil.plan).parameters
    assert callable(stencil.set_solve_check) and callable(stencil.get_solve_check)


def phases(x, y, px, py, rank, T, residual=False):
    from smi_amd import stencil
    return stencil.plan(x, y, px, py, rank, T, residual=residual)


def test_plan_residual_single_tile_k20(lib, restore_settings):
    """steps_per_pass 20 on 96x128, 1x1: the final pass is K_r = 12 steps (the
    residual lives in the K <= 12 sweep) after what smi_stencil_plan gives for
    the steps before it; short runs are one pass; fewer than 3 steps end in a
    single residual step."""
    from smi_amd import stencil
    stencil.set_fusion(steps_per_pass=20)
    before = phases(96, 128, 1, 1, 0, 29)
    assert before["phases"] == [(15, 1), (14, 1)]           # what run plans for 41 - 12 steps
    got = phases(96, 128, 1, 1, 0, 41, residual=True)
    assert got["phases"] == before["phases"] + [(12, 1)]
    assert got["result_index"] == 3 % 2
    assert got["neighbours"] == [-1] * 8
    assert phases(96, 128, 1, 1, 0, 5, residual=True)["phases"] == [(5, 1)]
    assert phases(96, 128, 1, 1, 0, 12, residual=True)["phases"] == [(12, 1)]
    assert phases(96, 128, 1, 1, 0, 13, residual=True)["phases"] == [(1, 1), (12, 1)]
    two = phases(96, 128, 1, 1, 0, 2, residual=True)
    assert two["phases"] == [(1, 1), (1, 1)] and two["result_index"] == 0
    assert phases(96, 128, 1, 1, 0, 1, residual=True)["phases"] == [(1, 1)]
    # the final pass is a phase of its own even where the phase before has the same depth
    stencil.set_fusion(steps_per_pass=12)
    assert phases(96, 128, 1, 1, 0, 36, residual=True)["phases"] == [(12, 2), (12, 1)]


@pytest.mark.parametrize("k", [1, 2])
def test_plan_residual_small_fusion_ends_in_a_single_step(lib, restore_settings, k):
    from smi_amd import stencil
    stencil.set_fusion(steps_per_pass=k)
    got = phases(96, 128, 1, 1, 0, 41, residual=True)["phases"]
    assert got == phases(96, 128, 1, 1, 0, 40)["phases"] + [(1, 1)]
    assert got[-1] == (1, 1)
    assert got[0] == ((2, 20) if k == 2 else (1, 40))


def test_plan_residual_clips_like_run_on_a_multi_rank_tile(lib, restore_settings):
    """A 16x32 tile of a 2x2 decomposition holds K-step passes of at most half
    its smaller side, 8 steps: smi_stencil_run clips to that, and so does the
    final residual pass (not 12)."""
    from smi_amd import stencil
    stencil.set_fusion(steps_per_pass=20)
    for rank in range(4):
        run = phases(16, 32, 2, 2, rank, 40)
        assert run["phases"] == [(8, 5)]
        res = phases(16, 32, 2, 2, rank, 41, residual=True)
        assert res["phases"] == phases(16, 32, 2, 2, rank, 33)["phases"] + [(8, 1)]
        assert res["neighbours"] == run["neighbours"]
        assert res["result_index"] == sum(n for _, n in res["phases"]) % 2
    # tiles too small for any K-step pass run single steps only
    assert phases(2, 4, 2, 2, 0, 7, residual=True)["phases"] == [(1, 6), (1, 1)]


def test_plan_residual_needs_no_more_than_four_phases(lib, restore_settings):
    from smi_amd import stencil
    worst = 0
    for k in range(1, 21):
        stencil.set_fusion(steps_per_pass=k)
        for T in range(1, 90):
            for args in ((96, 128, 1, 1, 0), (32, 64, 3, 3, 4), (200, 64, 1, 1, 0)):
                got = phases(*args, T, residual=True)["phases"]       # the binding passes max_phases = 4
                assert sum(s * n for s, n in got) == T
                assert got[-1][1] == 1 and got[-1][0] <= 12
                worst = max(worst, len(got))
    assert 3 <= worst <= 4


def test_bad_arguments_are_refused_before_any_device(lib, restore_settings):
    from smi_amd import SMIError, _lib, stencil
    with pytest.raises(SMIError):
        stencil.plan(96, 128, 1, 1, 0, 0, residual=True)             # a residual run takes >= 1 step
    assert "at least one step" in lib.smi_last_error().decode()
    buf = (ctypes.c_float * 64)()
    b0 = (ctypes.addressof(buf) + 15) // 16 * 16
    b1 = b0 + 32 * 4
    idx = ctypes.c_int(-7)
    bogus = _lib.SMI_Comm(0, 1, 987654)
    rc = lib.smi_stencil_run_residual(bogus, b0, b1, 2, 4, 1, 1, 5, b1, None, ctypes.byref(idx))
    assert rc == SMI_ERR_BAD_COMM and idx.value == -7
    assert lib.smi_stencil_set_solve_check(2) == SMI_ERR_INVALID_ARG
    stencil.set_solve_check(1)
    assert stencil.get_solve_check() == 1
    stencil.set_solve_check(-1)
    assert stencil.get_solve_check() == 1
    stencil.set_solve_check(0)
    assert stencil.get_solve_check() == 0


def test_solve_check_defaults_to_zero_in_a_fresh_process(lib):
    out = subprocess.run([sys.executable, "-c",
                          "import sys; sys.path.insert(0, sys.argv[1]); import smi_amd; smi_amd.load(); "
                          "from smi_amd import stencil; print('CHECK', stencil.get_solve_check())", ROOT],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "CHECK 0" in out.stdout
