"""smi_stencil_solve / smi_stencil_step_residual on the host, no GPU needed:
the symbols are declared, exported and bound, and the scalar arguments of
smi_stencil_solve are refused before any device or communicator is touched."""
import ctypes
import math
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("smi_stencil_step_residual", "smi_stencil_solve")
SMI_ERR_INVALID_ARG, SMI_ERR_BAD_COMM = -1, -5   # include/smi/status.h


@pytest.fixture(scope="module")
def lib():
    from smi_amd import _lib
    return _lib.load()


def test_symbols_declared_exported_bound(lib):
    from smi_amd import _lib, stencil
    header = open(os.path.join(ROOT, "include", "smi", "stencil.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW:
        assert re.search(rf"\bint\s+{name}\s*\(", header), name
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES["smi_stencil_step_residual"][1]) == 10
    assert len(_lib.SIGNATURES["smi_stencil_solve"][1]) == 15
    assert callable(stencil.solve)
    import inspect
    assert "residual" in inspect.signature(stencil.step).parameters
    assert list(inspect.signature(stencil.solve).parameters)[:5] == ["comm", "tile", "tol", "max_steps",
                                                                     "check_every"]


def _solve(lib, comm, tol, max_steps, check_every):
    """Raw call with well-formed buffers (host memory: never dereferenced,
    the call is refused first) and outputs."""
    buf = (ctypes.c_float * 64)()
    base = ctypes.addressof(buf)
    b0 = (base + 15) // 16 * 16
    b1 = b0 + 32 * 4
    idx, steps, conv = ctypes.c_int(-7), ctypes.c_int(-7), ctypes.c_int(-7)
    res = ctypes.c_float(-7.0)
    rc = lib.smi_stencil_solve(comm, b0, b1, 2, 4, 1, 1, ctypes.c_float(tol), max_steps, check_every, None,
                               ctypes.byref(idx), ctypes.byref(steps), ctypes.byref(res), ctypes.byref(conv))
    return rc, (idx.value, steps.value, res.value, conv.value)


@pytest.mark.parametrize("tol,max_steps,check_every,word", [
    (-1e-3, 10, 1, "tol"), (-0.0 - 1e-30, 10, 1, "tol"), (math.nan, 10, 1, "tol"), (1e-3, 10, 0, "check_every"),
    (1e-3, 10, -3, "check_every"), (1e-3, -1, 1, "max_steps")])
def test_bad_scalar_arguments_are_invalid_arg(lib, tol, max_steps, check_every, word):
    """Refused as SMI_ERR_INVALID_ARG with a message, before the communicator
    (an unknown one here) or any device is looked at; no output is written."""
    from smi_amd import _lib
    bogus = _lib.SMI_Comm(0, 1, 987654)
    rc, outs = _solve(lib, bogus, tol, max_steps, check_every)
    assert rc == SMI_ERR_INVALID_ARG
    msg = lib.smi_last_error().decode()
    assert "invalid argument" in msg and word in msg, msg
    assert outs == (-7, -7, -7.0, -7)


def test_valid_arguments_unknown_comm_fails_loudly(lib):
    """Well-formed arguments and no such communicator (without a GPU none can
    be made): SMI_ERR_BAD_COMM, and the Python mirror raises."""
    from smi_amd import SMIError, _lib
    bogus = _lib.SMI_Comm(0, 1, 987654)
    rc, _ = _solve(lib, bogus, 1e-3, 10, 1)
    assert rc == SMI_ERR_BAD_COMM
    assert "unknown communicator" in lib.smi_last_error().decode()
    rc, _ = _solve(lib, bogus, 0.0, 0, 1)   # tol = 0 and max_steps = 0 are valid
    assert rc == SMI_ERR_BAD_COMM
    with pytest.raises(SMIError):
        _lib.call("smi_stencil_solve", bogus, None, None, 2, 4, 1, 1, ctypes.c_float(1e-3), 10, 1, None,
                  ctypes.byref(ctypes.c_int()), ctypes.byref(ctypes.c_int()), ctypes.byref(ctypes.c_float()),
                  None)


def test_step_residual_rejects_bad_arguments_before_launch(lib):
    """smi_stencil_step_residual checks the tile like smi_stencil_step and
    needs a residual word."""
    buf = (ctypes.c_float * 64)()
    b0 = (ctypes.addressof(buf) + 15) // 16 * 16
    b1 = b0 + 32 * 4
    mode = (ctypes.c_int * 4)(0, 0, 0, 0)
    halo = (ctypes.c_void_p * 4)()
    # y_local % 4 != 0
    assert lib.smi_stencil_step_residual(b0, b1, 2, 6, mode, halo, None, None, b1, None) == SMI_ERR_INVALID_ARG
    # NULL residual word
    assert lib.smi_stencil_step_residual(b0, b1, 2, 4, mode, halo, None, None, None, None) == SMI_ERR_INVALID_ARG
    assert "resid_bits" in lib.smi_last_error().decode()
    # misaligned residual word
    assert lib.smi_stencil_step_residual(b0, b1, 2, 4, mode, halo, None, None, b1 + 2, None) == SMI_ERR_INVALID_ARG
