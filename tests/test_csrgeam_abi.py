"""CPU-side checks of the sparse-addition boundary (spg_csrgeam_nnz / spg_csrgeam,
include/spgemm.h): declared, exported, bound with prototypes, NULL handle rejected with a status,
the library still 0.2.0 with nine phases, and both routine names known to
cusparse.check_availability."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "spgemm.h")
LIB = os.path.join(ROOT, "spmm_amd", "lib", "libmi355_spgemm.so")


def test_header_declares_both_entry_points():
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    w = r"\s*\w+\s*"
    assert re.search(r"\bspg_status_t\s+spg_csrgeam_nnz\s*\(\s*spg_handle_t" + w + r",\s*const\s+spg_csr_t\s*\*" + w +
                     r",\s*const\s+spg_csr_t\s*\*" + w + r",\s*void\s*\*" + w + r",\s*spg_index_t" + w +
                     r",\s*int64_t\s*\*" + w + r",\s*size_t\s*\*" + w + r",\s*void\s*\*" + w + r"\)", src)
    assert re.search(r"\bspg_status_t\s+spg_csrgeam\s*\(\s*spg_handle_t" + w + r",\s*const\s+void\s*\*" + w +
                     r",\s*const\s+spg_csr_t\s*\*" + w + r",\s*const\s+void\s*\*" + w +
                     r",\s*const\s+spg_csr_t\s*\*" + w + r",\s*spg_csr_t\s*\*" + w + r",\s*size_t" + w +
                     r",\s*void\s*\*" + w + r"\)", src)
    assert "cusparseXcsrgeam2Nnz" in text and "csrgeam2_bufferSizeExt" in text
    assert "cupyx/cusparse.py:525-591" in text
    assert "Added within" in text.split("cusparseXcsrgeam2Nnz")[1].split("spg_status_t spg_csrgeam_nnz")[0]
    assert re.search(r"SPG_NUM_PHASES\s*=\s*9\b", src)
    assert re.search(r"SPG_VERSION_MINOR\s+2\b", src) and re.search(r"SPG_VERSION_PATCH\s+0\b", src)


def test_library_exports_both_symbols():
    assert os.path.exists(LIB), "run __graft_entry__.build() first"
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True,
                         check=True).stdout
    assert re.search(r"\bT spg_csrgeam_nnz\b", out)
    assert re.search(r"\bT spg_csrgeam\b", out)


def test_bindings_have_prototypes():
    from spmm_amd import _lib
    assert "spg_csrgeam_nnz" in _lib.EXPORTS and "spg_csrgeam" in _lib.EXPORTS
    lib = _lib.load()
    csrp = ctypes.POINTER(_lib.SpgCsr)
    assert lib.spg_csrgeam_nnz.restype is ctypes.c_int and lib.spg_csrgeam.restype is ctypes.c_int
    a = lib.spg_csrgeam_nnz.argtypes
    assert len(a) == 8 and a[1] is csrp and a[2] is csrp
    assert a[5] is ctypes.POINTER(ctypes.c_int64) and a[6] is ctypes.POINTER(ctypes.c_size_t)
    a = lib.spg_csrgeam.argtypes
    assert len(a) == 8 and a[2] is csrp and a[4] is csrp and a[5] is csrp and a[6] is ctypes.c_size_t
    assert len(_lib.PHASES) == _lib.NUM_PHASES == 9


def test_null_handle_is_not_initialized():
    from spmm_amd import _lib
    lib = _lib.load()
    assert lib.spg_csrgeam_nnz(None, None, None, None, 0, None, None, None) == 1   # NOT_INITIALIZED
    assert lib.spg_csrgeam(None, None, None, None, None, None, 0, None) == 1
    assert lib.spg_version() == 200                                                # additive within 0.2.0


def test_check_availability_knows_both_names():
    from spmm_amd import cusparse
    assert isinstance(cusparse.check_availability("csrgeam2"), bool)
    assert isinstance(cusparse.check_availability("csrgeam"), bool)
    assert cusparse.csrgeam is cusparse.csrgeam2
    assert cusparse.has_csrgeam() is True
