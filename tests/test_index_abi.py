"""CPU-side checks of the submatrix-extraction boundary (spg_csr_extract_nnz / spg_csr_extract and
spg_sel_t, include/spgemm.h): declared, exported, bound with prototypes, NULL handle rejected with
a status, the library still 0.2.0 with nine phases, and the routine name known to
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
    assert re.search(r"typedef\s+struct\s*\{\s*int64_t\s+start\s*,\s*step\s*,\s*count\s*;\s*const\s+int32_t\s*\*\s*index\s*;"
                     r"\s*\}\s*spg_sel_t\s*;", src)
    assert re.search(r"\bspg_status_t\s+spg_csr_extract_nnz\s*\(\s*spg_handle_t" + w + r",\s*const\s+spg_csr_t\s*\*" + w +
                     r",\s*const\s+spg_sel_t\s*\*" + w + r",\s*const\s+spg_sel_t\s*\*" + w + r",\s*void\s*\*" + w +
                     r",\s*spg_index_t" + w + r",\s*int64_t\s*\*" + w + r",\s*size_t\s*\*" + w + r",\s*void\s*\*" + w +
                     r"\)", src)
    assert re.search(r"\bspg_status_t\s+spg_csr_extract\s*\(\s*spg_handle_t" + w + r",\s*const\s+spg_csr_t\s*\*" + w +
                     r",\s*const\s+spg_sel_t\s*\*" + w + r",\s*const\s+spg_sel_t\s*\*" + w + r",\s*spg_csr_t\s*\*" + w +
                     r",\s*size_t" + w + r",\s*void\s*\*" + w + r"\)", src)
    comment = text.split("Submatrix extraction")[1].split("typedef struct { int64_t start")[0]
    for site in ("_index.py:348", ":45-115", "_compressed.py:403", ":566", ":643", ":665"):
        assert site in comment, site
    assert "Added within 0.2.0: a caller detects it by symbol lookup" in comment
    assert "k_ex_mark" in text and "k_ex_fill" in text
    assert re.search(r"SPG_NUM_PHASES\s*=\s*9\b", src)
    assert re.search(r"SPG_VERSION_MINOR\s+2\b", src) and re.search(r"SPG_VERSION_PATCH\s+0\b", src)


def test_library_exports_both_symbols():
    assert os.path.exists(LIB), "run __graft_entry__.build() first"
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True,
                         check=True).stdout
    assert re.search(r"\bT spg_csr_extract_nnz\b", out)
    assert re.search(r"\bT spg_csr_extract\b", out)


def test_bindings_have_prototypes():
    from spmm_amd import _lib
    assert "spg_csr_extract_nnz" in _lib.EXPORTS and "spg_csr_extract" in _lib.EXPORTS
    lib = _lib.load()
    csrp, selp = ctypes.POINTER(_lib.SpgCsr), ctypes.POINTER(_lib.SpgSel)
    assert [f[0] for f in _lib.SpgSel._fields_] == ["start", "step", "count", "index"]
    assert ctypes.sizeof(_lib.SpgSel) == 32
    assert lib.spg_csr_extract_nnz.restype is ctypes.c_int and lib.spg_csr_extract.restype is ctypes.c_int
    a = lib.spg_csr_extract_nnz.argtypes
    assert len(a) == 9 and a[1] is csrp and a[2] is selp and a[3] is selp and a[5] is ctypes.c_int
    assert a[6] is ctypes.POINTER(ctypes.c_int64) and a[7] is ctypes.POINTER(ctypes.c_size_t)
    a = lib.spg_csr_extract.argtypes
    assert len(a) == 7 and a[1] is csrp and a[2] is selp and a[3] is selp and a[4] is csrp and a[5] is ctypes.c_size_t
    assert len(_lib.PHASES) == _lib.NUM_PHASES == 9


def test_null_handle_is_not_initialized():
    from spmm_amd import _lib
    lib = _lib.load()
    assert lib.spg_csr_extract_nnz(None, None, None, None, None, 0, None, None, None) == 1   # NOT_INITIALIZED
    assert lib.spg_csr_extract(None, None, None, None, None, 0, None) == 1
    assert lib.spg_version() == 200                                                          # additive within 0.2.0


def test_check_availability_knows_the_name():
    from spmm_amd import cusparse
    assert isinstance(cusparse.check_availability("extract"), bool)
    assert cusparse.has_extract() is True
    assert "extract" in cusparse.__all__
