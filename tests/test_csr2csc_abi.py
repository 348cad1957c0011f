"""CPU-side checks of the transpose boundary (spg_csr2csc, include/spgemm.h): declared, exported,
bound with a prototype, NULL handle rejected with a status, the library still 0.2.0, and the two
routine names known to cusparse.check_availability."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "spgemm.h")
LIB = os.path.join(ROOT, "spmm_amd", "lib", "libmi355_spgemm.so")


def test_header_declares_spg_csr2csc():
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bspg_status_t\s+spg_csr2csc\s*\(\s*spg_handle_t\s+\w+\s*,\s*const\s+spg_csr_t\s*\*\s*\w+\s*,"
                     r"\s*spg_csr_t\s*\*\s*\w+\s*,\s*size_t\s*\*\s*\w+\s*,\s*void\s*\*\s*\w+\s*\)", src)
    assert "cusparseCsr2cscEx2" in text and "cupyx/cusparse.py:1014-1065" in text
    assert re.search(r"SPG_NUM_PHASES\s*=\s*9\b", src)


def test_library_exports_spg_csr2csc():
    assert os.path.exists(LIB), "run __graft_entry__.build() first"
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True,
                         check=True).stdout
    assert re.search(r"\bT spg_csr2csc\b", out)


def test_binding_has_prototype():
    from spmm_amd import _lib
    assert "spg_csr2csc" in _lib.EXPORTS
    lib = _lib.load()
    assert lib.spg_csr2csc.restype is ctypes.c_int
    assert len(lib.spg_csr2csc.argtypes) == 5
    assert lib.spg_csr2csc.argtypes[1] is ctypes.POINTER(_lib.SpgCsr)
    assert lib.spg_csr2csc.argtypes[2] is ctypes.POINTER(_lib.SpgCsr)
    assert lib.spg_csr2csc.argtypes[3] is ctypes.POINTER(ctypes.c_size_t)
    assert len(_lib.PHASES) == _lib.NUM_PHASES == 9


def test_null_handle_is_not_initialized():
    from spmm_amd import _lib
    lib = _lib.load()
    assert lib.spg_csr2csc(None, None, None, None, None) == 1   # NOT_INITIALIZED
    assert lib.spg_version() == 200                             # additive within 0.2.0


def test_check_availability_knows_both_names():
    from spmm_amd import cusparse
    assert isinstance(cusparse.check_availability("csr2csc"), bool)
    assert isinstance(cusparse.check_availability("csc2csr"), bool)
