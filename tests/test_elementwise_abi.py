"""CPU-side checks of the element-wise boundary (spg_csr_binop_nnz / spg_csr_binop /
spg_csr_mul_dense, include/spgemm.h): declared with the reference's lines cited, exported, bound with
exact prototypes, a NULL handle rejected with a status by each, the library still 0.2.0 with nine
phases.  An unknown op needs a live handle to get past the handle check, so that one test is
marked gpu."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "spgemm.h")
LIB = os.path.join(ROOT, "spmm_amd", "lib", "libmi355_spgemm.so")
NAMES = ("spg_csr_binop_nnz", "spg_csr_binop", "spg_csr_mul_dense")


def test_header_declares_the_three_entry_points():
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    w = r"\s*\w+\s*"
    csr, dn = r",\s*const\s+spg_csr_t\s*\*" + w, r",\s*const\s+spg_dense_t\s*\*" + w
    assert re.search(r"typedef\s+enum\s*\{\s*SPG_BINOP_MUL\s*=\s*0\s*,\s*SPG_BINOP_MAX\s*=\s*1\s*,\s*SPG_BINOP_MIN\s*=\s*2\s*\}"
                     r"\s*spg_binop_t\s*;", src)
    assert re.search(r"\bspg_status_t\s+spg_csr_binop_nnz\s*\(\s*spg_handle_t" + w + r",\s*spg_binop_t" + w + csr + csr +
                     r",\s*void\s*\*" + w + r",\s*spg_index_t" + w + r",\s*int64_t\s*\*" + w + r",\s*size_t\s*\*" + w +
                     r",\s*void\s*\*" + w + r"\)", src)
    assert re.search(r"\bspg_status_t\s+spg_csr_binop\s*\(\s*spg_handle_t" + w + r",\s*spg_binop_t" + w + csr + csr +
                     r",\s*spg_csr_t\s*\*" + w + r",\s*size_t" + w + r",\s*void\s*\*" + w + r"\)", src)
    assert re.search(r"\bspg_status_t\s+spg_csr_mul_dense\s*\(\s*spg_handle_t" + w + r",\s*const\s+spg_csr_t\s*\*" + w + dn +
                     r",\s*void\s*\*" + w + r"\)", src)
    # the reference's lines: multiply, _maximum_minimum and the three kernels
    binop_doc = text.split("spg_status_t spg_csr_binop_nnz")[0].split("spg_status_t spg_csrgeam(")[1]
    assert "cupyx/scipy/sparse/_csr.py:328-342" in binop_doc and ":297-326" in binop_doc
    assert ":733-835" in binop_doc and ":880-945" in binop_doc and "Added within" in binop_doc
    assert "must not change between the two calls" in binop_doc and "SPG_CANON_DROP_ZEROS" in binop_doc
    dense_doc = text.split("spg_status_t spg_csr_mul_dense")[0].split("spg_status_t spg_csr_binop(")[1]
    assert "_csr.py:617-718" in dense_doc and "Added within" in dense_doc
    assert re.search(r"SPG_NUM_PHASES\s*=\s*9\b", src)
    assert re.search(r"SPG_VERSION_MINOR\s+2\b", src) and re.search(r"SPG_VERSION_PATCH\s+0\b", src)


def test_library_exports_the_symbols():
    assert os.path.exists(LIB), "run __graft_entry__.build() first"
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    for name in NAMES:
        assert re.search(r"\bT " + name + r"\b", out), name


def test_bindings_have_exact_prototypes():
    from spmm_amd import _lib
    assert _lib.ELEMENTWISE == NAMES and all(n in _lib.EXPORTS for n in NAMES)
    assert (_lib.SPG_BINOP_MUL, _lib.SPG_BINOP_MAX, _lib.SPG_BINOP_MIN) == (0, 1, 2)
    lib = _lib.load()
    vp, csrp, dnp = ctypes.c_void_p, ctypes.POINTER(_lib.SpgCsr), ctypes.POINTER(_lib.SpgDense)
    i64p, szp = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_size_t)
    assert all(getattr(lib, n).restype is ctypes.c_int for n in NAMES)
    assert lib.spg_csr_binop_nnz.argtypes == [vp, ctypes.c_int, csrp, csrp, vp, ctypes.c_int, i64p, szp, vp]
    assert lib.spg_csr_binop.argtypes == [vp, ctypes.c_int, csrp, csrp, csrp, ctypes.c_size_t, vp]
    assert lib.spg_csr_mul_dense.argtypes == [vp, csrp, dnp, vp]
    assert len(_lib.PHASES) == _lib.NUM_PHASES == 9


def test_null_handle_is_not_initialized():
    from spmm_amd import _lib
    lib = _lib.load()
    assert lib.spg_csr_binop_nnz(None, 0, None, None, None, 0, None, None, None) == 1   # NOT_INITIALIZED
    assert lib.spg_csr_binop_nnz(None, 7, None, None, None, 0, None, None, None) == 1   # (before the op is looked at)
    assert lib.spg_csr_binop(None, 0, None, None, None, 0, None) == 1
    assert lib.spg_csr_mul_dense(None, None, None, None) == 1
    assert lib.spg_version() == 200                                                     # additive within 0.2.0


def test_has_elementwise():
    from spmm_amd import cusparse
    assert cusparse.has_elementwise() is True
    assert set(cusparse._BINOPS) == {"multiply", "maximum", "minimum"}


@pytest.mark.gpu
def test_unknown_op_is_invalid_value():
    torch = pytest.importorskip("torch")
    from spmm_amd import _lib
    h = _lib.get_handle(0)
    p = torch.zeros(3, dtype=torch.int32, device="cuda:0")
    v = _lib.SpgCsr(2, 2, 0, p.data_ptr(), 0, 0, _lib.SPG_INDEX_32I, _lib.SPG_R_64F)
    nnz, need = ctypes.c_int64(-1), ctypes.c_size_t(0)
    for op in (3, -1, 100):
        assert h.lib.spg_csr_binop_nnz(h.ptr, op, ctypes.byref(v), ctypes.byref(v), None, _lib.SPG_INDEX_32I,
                                       ctypes.byref(nnz), ctypes.byref(need), None) == 3      # INVALID_VALUE
        assert h.lib.spg_csr_binop(h.ptr, op, ctypes.byref(v), ctypes.byref(v), ctypes.byref(v), 4096,
                                   ctypes.c_void_p(p.data_ptr())) == 3
    assert need.value == 0
    assert h.lib.spg_csr_binop_nnz(h.ptr, 2, ctypes.byref(v), ctypes.byref(v), None, _lib.SPG_INDEX_32I,
                                   ctypes.byref(nnz), ctypes.byref(need), None) == 0 and need.value > 0
