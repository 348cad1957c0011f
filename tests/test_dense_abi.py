"""CPU-side checks of the dense boundary (spg_csr2dense, spg_dense2csr_nnz, spg_dense2csr;
include/spgemm.h): declared with the cupyx lines they replace, exported, bound with prototypes,
NULL handle rejected with a status, the library still 0.2.0 with 9 phases, and the header and
the binding still list the same symbols."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "spgemm.h")
LIB = os.path.join(ROOT, "spmm_amd", "lib", "libmi355_spgemm.so")
NAMES = ("spg_csr2dense", "spg_dense2csr_nnz", "spg_dense2csr")


def _arg(t):
    return r"\s*" + t.replace(" ", r"\s+").replace("*", r"\s*\*\s*") + r"\s*\w+\s*"


def test_header_declares_the_three_prototypes():
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    protos = {
        "spg_csr2dense": ["spg_handle_t ", "const spg_csr_t *", "spg_dense_t *"],
        "spg_dense2csr_nnz": ["spg_handle_t ", "const spg_dense_t *", "void *", "spg_index_t ", "int64_t *",
                              "size_t *", "void *"],
        "spg_dense2csr": ["spg_handle_t ", "const spg_dense_t *", "spg_csr_t *", "size_t ", "void *"],
    }
    for name, args in protos.items():
        pat = r"\bspg_status_t\s+" + name + r"\s*\(" + ",".join(_arg(a.strip()) for a in args) + r"\)\s*;"
        assert re.search(pat, src), name
    # the cupyx lines each entry point replaces
    for ref in ("cupyx/cusparse.py:768-797", ":800-829", ":1805-1833", "cupyx/scipy/sparse/_csr.py:383-428",
                "cupyx/cusparse.py:1188-1228", ":1146-1185", ":1733-1802", "cupyx/scipy/sparse/_csr.py:60-80",
                ":1158-1210", "cusparseSparseToDense", "cusparseDenseToSparse"):
        assert ref in text, ref
    assert re.search(r"SPG_NUM_PHASES\s*=\s*9\b", src)
    assert re.search(r"SPG_VERSION_MINOR\s+2\b", src) and re.search(r"SPG_VERSION_PATCH\s+0\b", src)


def test_library_exports_the_symbols():
    assert os.path.exists(LIB), "run __graft_entry__.build() first"
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    for name in NAMES:
        assert re.search(r"\bT " + name + r"\b", out), name


def test_binding_has_prototypes():
    from spmm_amd import _lib, cusparse
    lib = _lib.load()
    csrp, dnp = ctypes.POINTER(_lib.SpgCsr), ctypes.POINTER(_lib.SpgDense)
    for name in NAMES:
        assert name in _lib.EXPORTS
        assert getattr(lib, name).restype is ctypes.c_int
    assert lib.spg_csr2dense.argtypes == [ctypes.c_void_p, csrp, dnp]
    assert lib.spg_dense2csr_nnz.argtypes == [ctypes.c_void_p, dnp, ctypes.c_void_p, ctypes.c_int,
                                             ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_size_t),
                                             ctypes.c_void_p]
    assert lib.spg_dense2csr.argtypes == [ctypes.c_void_p, dnp, csrp, ctypes.c_size_t, ctypes.c_void_p]
    assert cusparse.has_dense_convert() is True
    assert len(_lib.PHASES) == _lib.NUM_PHASES == 9


def test_null_handle_is_not_initialized():
    from spmm_amd import _lib
    lib = _lib.load()
    assert lib.spg_csr2dense(None, None, None) == 1                              # NOT_INITIALIZED, checked first
    assert lib.spg_dense2csr_nnz(None, None, None, 32, None, None, None) == 1
    assert lib.spg_dense2csr(None, None, None, 0, None) == 1
    assert lib.spg_version() == 200                                              # additive within 0.2.0


def test_header_and_binding_list_the_same_symbols():
    from spmm_amd import _lib
    from tests.test_abi import declared_functions
    assert set(_lib.EXPORTS) == set(declared_functions())
    assert set(NAMES) <= set(declared_functions())
