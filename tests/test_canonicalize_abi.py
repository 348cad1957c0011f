"""CPU-side checks of the canonicalisation boundary (spg_canonicalize_nnz / spg_canonicalize,
include/spgemm.h): declared, exported, bound with prototypes, NULL handle rejected with a status,
the library still 0.2.0 with nine phases, and the routine names known to
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
    assert re.search(r"\bspg_status_t\s+spg_canonicalize_nnz\s*\(\s*spg_handle_t" + w +
                     r",\s*const\s+spg_csr_t\s*\*" + w + r",\s*const\s+int32_t\s*\*" + w + r",\s*unsigned" + w +
                     r",\s*void\s*\*" + w + r",\s*spg_index_t" + w + r",\s*int64_t\s*\*" + w +
                     r",\s*size_t\s*\*" + w + r",\s*void\s*\*" + w + r"\)", src)
    assert re.search(r"\bspg_status_t\s+spg_canonicalize\s*\(\s*spg_handle_t" + w +
                     r",\s*const\s+spg_csr_t\s*\*" + w + r",\s*const\s+int32_t\s*\*" + w + r",\s*unsigned" + w +
                     r",\s*spg_csr_t\s*\*" + w + r",\s*size_t" + w + r",\s*void\s*\*" + w + r"\)", src)
    assert re.search(r"SPG_CANON_SORT\s*=\s*1\s*,\s*SPG_CANON_SUM\s*=\s*2\s*,\s*SPG_CANON_DROP_ZEROS\s*=\s*4", src)
    comment = text.split("cusparseXcsrsort")[1].split("spg_status_t spg_canonicalize_nnz")[0]
    assert "Added within" in comment and "cupyx/cusparse.py:832-867" in comment
    assert re.search(r"SPG_NUM_PHASES\s*=\s*9\b", src)
    assert re.search(r"SPG_VERSION_MINOR\s+2\b", src) and re.search(r"SPG_VERSION_PATCH\s+0\b", src)


def test_library_exports_both_symbols():
    assert os.path.exists(LIB), "run __graft_entry__.build() first"
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True,
                         check=True).stdout
    assert re.search(r"\bT spg_canonicalize_nnz\b", out)
    assert re.search(r"\bT spg_canonicalize\b", out)


def test_bindings_have_prototypes():
    from spmm_amd import _lib
    assert "spg_canonicalize_nnz" in _lib.EXPORTS and "spg_canonicalize" in _lib.EXPORTS
    assert (_lib.SPG_CANON_SORT, _lib.SPG_CANON_SUM, _lib.SPG_CANON_DROP_ZEROS) == (1, 2, 4)
    lib = _lib.load()
    csrp = ctypes.POINTER(_lib.SpgCsr)
    assert lib.spg_canonicalize_nnz.restype is ctypes.c_int and lib.spg_canonicalize.restype is ctypes.c_int
    a = lib.spg_canonicalize_nnz.argtypes
    assert len(a) == 9 and a[1] is csrp and a[3] is ctypes.c_uint
    assert a[6] is ctypes.POINTER(ctypes.c_int64) and a[7] is ctypes.POINTER(ctypes.c_size_t)
    a = lib.spg_canonicalize.argtypes
    assert len(a) == 7 and a[1] is csrp and a[3] is ctypes.c_uint and a[4] is csrp and a[5] is ctypes.c_size_t
    assert len(_lib.PHASES) == _lib.NUM_PHASES == 9


def test_null_handle_is_not_initialized():
    from spmm_amd import _lib
    lib = _lib.load()
    assert lib.spg_canonicalize_nnz(None, None, None, 0, None, 0, None, None, None) == 1   # NOT_INITIALIZED
    assert lib.spg_canonicalize(None, None, None, 0, None, 0, None) == 1
    assert lib.spg_version() == 200                                                        # additive within 0.2.0


def test_check_availability_knows_the_names():
    from spmm_amd import cusparse
    assert isinstance(cusparse.check_availability("canonicalize"), bool)
    assert isinstance(cusparse.check_availability("csrsort"), bool)
    assert cusparse.has_canonicalize() is True
    assert callable(cusparse.canonicalize) and callable(cusparse.csrsort)
