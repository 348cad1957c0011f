"""CPU-side checks of the SpMM boundary (spg_spmm, include/spgemm.h): declared, exported,
bound with a prototype, NULL handle rejected with a status, and a known routine name of
cusparse.check_availability."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "spgemm.h")
LIB = os.path.join(ROOT, "spmm_amd", "lib", "libmi355_spgemm.so")


def test_header_declares_spg_spmm():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bspg_status_t\s+spg_spmm\s*\(", src)
    assert re.search(r"\}\s*spg_dense_t\s*;", src)
    assert re.search(r"SPG_ORDER_COL\s*=\s*1\b", src) and re.search(r"SPG_ORDER_ROW\s*=\s*2\b", src)


def test_library_exports_spg_spmm():
    assert os.path.exists(LIB), "run __graft_entry__.build() first"
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True,
                         check=True).stdout
    assert re.search(r"\bT spg_spmm\b", out)


def test_binding_has_prototype():
    from spmm_amd import _lib
    assert "spg_spmm" in _lib.EXPORTS
    lib = _lib.load()
    assert lib.spg_spmm.restype is ctypes.c_int
    assert len(lib.spg_spmm.argtypes) == 6
    assert lib.spg_spmm.argtypes[2] is ctypes.POINTER(_lib.SpgDense)
    assert lib.spg_spmm.argtypes[5] is ctypes.POINTER(_lib.SpgDense)
    # spg_dense_t: three int64, a pointer, two enums
    assert ctypes.sizeof(_lib.SpgDense) == 40
    assert (_lib.SPG_ORDER_COL, _lib.SPG_ORDER_ROW) == (1, 2)


def test_null_handle_is_not_initialized():
    from spmm_amd import _lib
    lib = _lib.load()
    assert lib.spg_spmm(None, None, None, None, None, None) == 1   # NOT_INITIALIZED
    assert lib.spg_version() == 200                                # additive within 0.2.0


def test_check_availability_knows_spmm():
    from spmm_amd import cusparse
    assert isinstance(cusparse.check_availability("spmm"), bool)
