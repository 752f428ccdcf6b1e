"""smi_allreduce, smi_kmeans_means and smi_kmeans_set_means / _get_means on the
host, no GPU needed: the symbols are declared, exported and bound, an unknown
communicator is refused, and the means mode keeps its value under -1."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMI_ERR_INVALID_ARG, SMI_ERR_BAD_COMM = -1, -5   # include/smi/status.h
NEW = {"smi_allreduce": ("allreduce.h", 8), "smi_kmeans_means": ("kmeans.h", 9),
       "smi_kmeans_set_means": ("kmeans.h", 1), "smi_kmeans_get_means": ("kmeans.h", 1)}


@pytest.fixture(scope="module")
def lib():
    from smi_amd import _lib
    return _lib.load()


def test_symbols_declared_exported_bound(lib):
    from smi_amd import _lib, collectives, kmeans
    for name, (hdr, nargs) in NEW.items():
        header = open(os.path.join(ROOT, "include", "smi", hdr)).read()
        header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
        assert re.search(rf"\bint\s+{name}\s*\(", header), name
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
    umbrella = open(os.path.join(ROOT, "include", "smi.h")).read()
    assert '#include "smi/allreduce.h"' in umbrella
    import inspect
    assert list(inspect.signature(collectives.allreduce).parameters) == ["comm", "send", "recv", "op", "port",
                                                                         "stream"]
    assert inspect.signature(collectives.allreduce).parameters["recv"].default is None
    assert list(inspect.signature(kmeans.means).parameters) == ["sums", "counts", "out", "stream"]
    assert callable(kmeans.set_means)


def test_header_states_identical_results_on_every_rank():
    text = open(os.path.join(ROOT, "include", "smi", "allreduce.h")).read()
    flat = " ".join(text.replace("*", " ").split())
    assert "byte-identical" in flat and "same on every rank" in flat


def test_unknown_communicator_is_bad_comm(lib):
    """Checked first, as in smi_reduce; host memory is never dereferenced."""
    from smi_amd import SMIError, _lib
    bogus = _lib.SMI_Comm(0, 1, 987654)
    buf = (ctypes.c_float * 8)()
    p = ctypes.addressof(buf)
    rc = lib.smi_allreduce(bogus, p, p, 8, _lib.SMI_FLOAT, _lib.SMI_ADD, 0, None)
    assert rc == SMI_ERR_BAD_COMM
    assert "unknown communicator" in lib.smi_last_error().decode()
    with pytest.raises(SMIError):
        _lib.call("smi_allreduce", bogus, p, p, 8, _lib.SMI_FLOAT, _lib.SMI_ADD, 0, None)


def test_means_mode_default_and_keep(lib):
    from smi_amd import SMIError, kmeans
    v = ctypes.c_int(-7)
    assert lib.smi_kmeans_get_means(ctypes.byref(v)) == 0
    assert v.value == 0                      # the default: four collectives and a divide
    assert kmeans.set_means(-1) == 0         # -1 keeps it
    try:
        assert kmeans.set_means(1) == 1
        assert kmeans.set_means(-1) == 1
        assert lib.smi_kmeans_get_means(ctypes.byref(v)) == 0 and v.value == 1
        with pytest.raises(SMIError):
            kmeans.set_means(2)
        assert kmeans.set_means(-1) == 1     # a refused value changes nothing
    finally:
        kmeans.set_means(0)
    assert kmeans.set_means(-1) == 0


def test_means_rejects_bad_arguments_before_launch(lib):
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    # nranks 0 and 65, a row pitch below the row, NULL buffers
    assert lib.smi_kmeans_means(p, p, 0, 16, 4, 4, 4, p, None) == SMI_ERR_INVALID_ARG
    assert lib.smi_kmeans_means(p, p, 65, 16, 4, 4, 4, p, None) == SMI_ERR_INVALID_ARG
    assert lib.smi_kmeans_means(p, p, 2, 15, 4, 4, 4, p, None) == SMI_ERR_INVALID_ARG
    assert lib.smi_kmeans_means(p, p, 2, 16, 3, 4, 4, p, None) == SMI_ERR_INVALID_ARG
    assert lib.smi_kmeans_means(p, None, 2, 16, 4, 4, 4, p, None) == SMI_ERR_INVALID_ARG
    assert lib.smi_kmeans_means(p, p, 2, 16, 4, 4, 4, None, None) == SMI_ERR_INVALID_ARG
