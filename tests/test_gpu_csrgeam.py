"""Device sparse addition (spg_csrgeam_nnz / spg_csrgeam; cupyx.cusparse.csrgeam2,
modify_src/cupy-src/cupyx/cusparse.py:525-591) and the ``+`` / ``-`` / unary ``-`` operators of
the containers that run on it.

Bar (tests/geam_cases.py): C's indptr and indices equal scipy's sum of the two patterns with
all-ones values; after eliminate_zeros() on both sides the values equal scipy's under
special_values.assert_same_special, for the four value types, both row-pointer types of A and B
and both of C.

The kernels' seams (spmm_amd/csrc/spgemm_geam.hpp): a wave walks its chunk of GM_CHUNK = 1024
entries 64 at a time, a workgroup holds GM_WPB = 4 waves (4096 entries); a step whose 64 entries
lie in one row searches a window of the other row; the two scans work in tiles of SCAN_TILE = 2048.

Not tested here: SPG_STATUS_OVERFLOW (nnz(C) past an int32 row pointer) needs 2**31 entries;
tests/test_gpu_large_offsets.py::test_csrgeam has them, built on the device.

The complex `mixed` cases of test_special_values are what tells (1, -1), the subtraction, from
(2, -1): scipy's A - B subtracts part by part, while numpy's (-1) * B in (2*A) + (-1*B) is the
complex product with (-1, 0) and turns an infinite part of b into a NaN in its other part.
"""
import ctypes
import functools

import numpy as np
import pytest
import scipy.sparse as sp

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import geam_cases as gc          # noqa: E402
from tests import special_values as sv      # noqa: E402

DTYPES = gc.DTYPES
IPCP = [(np.int32, np.int32), (np.int32, np.int64), (np.int64, np.int32), (np.int64, np.int64)]
INVALID_VALUE, NOT_INITIALIZED = 3, 1
DEV = "cuda:0"


def _ipcp_id(v):
    return "A%d-C%d" % (np.dtype(v[0]).itemsize * 8, np.dtype(v[1]).itemsize * 8)


def _name(dt):
    return np.dtype(dt).name


class _Call:
    """One addition through ctypes on the scipy CSR pair (A, B), step by step.  fill: byte the
    workspace and the three output arrays hold before the calls; same: B's descriptor points at
    A's arrays."""

    def __init__(self, A, B, alpha=1, beta=1, ip=np.int32, cp=np.int32, fill=None, same=False):
        from spmm_amd import _lib
        from spmm_amd.cusparse import _IT, _VT, _alpha_of
        self.lib_mod = _lib
        self.h = _lib.get_handle(0)
        self.h.set_stream(torch.cuda.current_stream(0).cuda_stream)
        self.lib, self.fill = self.h.lib, fill
        self.shape = A.shape
        tip = torch.int32 if ip == np.int32 else torch.int64
        self.tcp = torch.int32 if cp == np.int32 else torch.int64
        self.keep = []

        def view(S):
            p = torch.from_numpy(S.indptr.astype(ip)).to(DEV)
            j = torch.from_numpy(S.indices.astype(np.int32)).to(DEV)
            x = torch.from_numpy(S.data.copy()).to(DEV)
            self.keep += [p, j, x]
            nnz = int(S.indptr[-1])
            return _lib.SpgCsr(S.shape[0], S.shape[1], nnz, p.data_ptr(), j.data_ptr() if nnz else 0,
                               x.data_ptr() if nnz else 0, _IT[tip], _VT[x.dtype]), x.dtype
        self.va, self.vdt = view(A)
        self.vb = self.va if same else view(B)[0]
        self.ctype = _IT[self.tcp]
        self.cp_t = self.buf(A.shape[0] + 1, self.tcp)
        self.al, self.be = _alpha_of(self.vdt, alpha), _alpha_of(self.vdt, beta)
        self.nnz = ctypes.c_int64(-1)
        self.need = ctypes.c_size_t(0)
        self.ws = None
        self.vc = None
        self._VT = _VT

    def buf(self, count, dtype):
        t = torch.empty(max(int(count), 1), dtype=dtype, device=DEV)
        if self.fill is not None:
            t.view(torch.uint8).fill_(self.fill)
        return t

    def query(self):
        return self.lib.spg_csrgeam_nnz(self.h.ptr, ctypes.byref(self.va), ctypes.byref(self.vb), None, self.ctype,
                                        ctypes.byref(self.nnz), ctypes.byref(self.need), None)

    def structure(self, shrink=0):
        self.ws = self.buf(self.need.value, torch.uint8)
        have = ctypes.c_size_t(self.need.value - shrink)
        return self.lib.spg_csrgeam_nnz(self.h.ptr, ctypes.byref(self.va), ctypes.byref(self.vb),
                                        ctypes.c_void_p(self.cp_t.data_ptr()), self.ctype, ctypes.byref(self.nnz),
                                        ctypes.byref(have), ctypes.c_void_p(self.ws.data_ptr()))

    def alloc_c(self):
        n = int(self.nnz.value)
        self.cj, self.cx = self.buf(n, torch.int32), self.buf(n, self.vdt)
        self.vc = self.lib_mod.SpgCsr(self.shape[0], self.shape[1], n, self.cp_t.data_ptr(),
                                      self.cj.data_ptr() if n else 0, self.cx.data_ptr() if n else 0, self.ctype,
                                      self._VT[self.vdt])

    def values(self, shrink=0):
        if self.vc is None:
            self.alloc_c()
        return self.lib.spg_csrgeam(self.h.ptr, ctypes.byref(self.al), ctypes.byref(self.va), ctypes.byref(self.be),
                                    ctypes.byref(self.vb), ctypes.byref(self.vc),
                                    ctypes.c_size_t(self.need.value - shrink), ctypes.c_void_p(self.ws.data_ptr()))

    def result(self):
        torch.cuda.synchronize()
        n = int(self.nnz.value)
        return self.cp_t[:self.shape[0] + 1].cpu().numpy(), self.cj[:n].cpu().numpy(), self.cx[:n].cpu().numpy()


def _run(A, B, alpha=1, beta=1, ip=np.int32, cp=np.int32, fill=None, same=False):
    c = _Call(A, B, alpha, beta, ip, cp, fill, same)
    assert c.query() == 0 and c.need.value > 0
    assert c.structure() == 0
    assert c.values() == 0
    got = c.result()
    assert got[0].dtype == cp and int(got[0][-1]) == c.nnz.value == got[1].size
    return got


@functools.lru_cache(maxsize=None)
def _ref(which, dt, alpha, beta):
    """scipy's result of a pair, computed once and never written."""
    A, B = {"edge": gc.edge_pair, "long": gc.long_pair}[which](dt)
    return gc.reference(A, B, alpha, beta)


# ------------------------------------------------------------------ 1. edge matrix
@pytest.mark.parametrize("ipcp", IPCP, ids=_ipcp_id)
@pytest.mark.parametrize("dt,coefs", gc.DTYPE_COEFS, ids=gc.case_id)
def test_edge_matrix(dt, coefs, ipcp):
    A, B = gc.edge_pair(dt)
    got = _run(A, B, *coefs, ip=ipcp[0], cp=ipcp[1])
    gc.assert_equal(got, A, B, *coefs, ref=_ref("edge", dt, *coefs))


# ------------------------------------------------------------------ 2. long rows
@pytest.mark.parametrize("ipcp", IPCP, ids=_ipcp_id)
@pytest.mark.parametrize("dt", DTYPES, ids=_name)
def test_long_rows(dt, ipcp):
    """Rows of 5,000, 9,000 and 30,000 entries: longer than a wave's chunk and a workgroup's
    entries, so most steps are one-row steps that search a window."""
    A, B = gc.long_pair(dt)
    coefs = (0.3, -2.7) if np.dtype(dt).kind != "c" else gc.COMPLEX_COEFS[0]
    got = _run(A, B, *coefs, ip=ipcp[0], cp=ipcp[1])
    gc.assert_equal(got, A, B, *coefs, ref=_ref("long", dt, *coefs))


# ------------------------------------------------------------------ 3. scan seams
@pytest.mark.parametrize("ipcp", IPCP, ids=_ipcp_id)
@pytest.mark.parametrize("nnz_b", [2047, 2048, 2049, 4097])
def test_scan_seams_entries(nnz_b, ipcp):
    """nnz(B) around one and two scan tiles (SCAN_TILE = 2048), nnz(A) different from nnz(B)."""
    A, B = gc.random_pair(300, 257, nnz_b + 101, nnz_b)
    assert B.nnz == nnz_b and A.nnz != B.nnz
    gc.assert_equal(_run(A, B, 1, -1, ip=ipcp[0], cp=ipcp[1]), A, B, 1, -1)


@pytest.mark.parametrize("ipcp", IPCP, ids=_ipcp_id)
@pytest.mark.parametrize("rows", [2047, 2048, 2049])
def test_scan_seams_rows(rows, ipcp):
    """The row scan at one tile and one row past it."""
    A, B = gc.random_pair(rows, 40, 5000, 4000)
    gc.assert_equal(_run(A, B, ip=ipcp[0], cp=ipcp[1]), A, B, 1, 1)


# ------------------------------------------------------------------ 4. degenerate sizes
@pytest.mark.parametrize("ipcp", IPCP, ids=_ipcp_id)
@pytest.mark.parametrize("shape", [(0, 0), (0, 5), (5, 0)])
def test_empty_shapes(shape, ipcp):
    E = sp.csr_matrix(shape, dtype=np.float64)
    p, j, x = _run(E, E, ip=ipcp[0], cp=ipcp[1], fill=0xFF)
    assert p.tolist() == [0] * (shape[0] + 1) and j.size == 0 and x.size == 0


@pytest.mark.parametrize("ipcp", IPCP, ids=_ipcp_id)
@pytest.mark.parametrize("empty", ["A", "B", "both"])
def test_empty_operands(empty, ipcp):
    """nnz(A) = 0 gives beta*B, nnz(B) = 0 alpha*A, both an all-zero row pointer."""
    A, B = gc.random_pair(70, 33, 500, 400)
    Z = sp.csr_matrix(A.shape, dtype=A.dtype)
    A, B = (Z if empty in ("A", "both") else A), (Z if empty in ("B", "both") else B)
    got = _run(A, B, 0.3, -2.7, ip=ipcp[0], cp=ipcp[1], fill=0xFF)
    gc.assert_equal(got, A, B, 0.3, -2.7)
    if empty == "both":
        assert not got[0].any() and got[1].size == 0
    if empty == "A":
        assert np.array_equal(got[2], np.float64(-2.7) * B.data)


@pytest.mark.parametrize("ipcp", IPCP, ids=_ipcp_id)
def test_one_by_one(ipcp):
    one, none = sp.csr_matrix(np.array([[2.5]])), sp.csr_matrix((1, 1), dtype=np.float64)
    for A, B, want in [(one, one, [5.0]), (one, none, [2.5]), (none, one, [2.5]), (none, none, [])]:
        p, j, x = _run(A, B, ip=ipcp[0], cp=ipcp[1], fill=0xFF)
        assert p.tolist() == [0, len(want)] and j.tolist() == [0] * len(want) and x.tolist() == want


# ------------------------------------------------------------------ 5. the same arrays twice
@pytest.mark.parametrize("ipcp", IPCP, ids=_ipcp_id)
@pytest.mark.parametrize("dt", DTYPES, ids=_name)
def test_same_arrays(dt, ipcp):
    A, _ = gc.edge_pair(dt)
    p, j, x = _run(A, A, 1, 1, ip=ipcp[0], cp=ipcp[1], same=True)
    assert np.array_equal(p, A.indptr) and np.array_equal(j, A.indices)
    assert np.array_equal(x.view(np.uint8), (A.data + A.data).view(np.uint8))
    p, j, x = _run(A, A, 1, -1, ip=ipcp[0], cp=ipcp[1], same=True, fill=0xFF)
    assert np.array_equal(p, A.indptr) and np.array_equal(j, A.indices)
    assert x.size == A.nnz and not x.view(np.uint8).any()


# ------------------------------------------------------------------ 6. poisoned buffers
@pytest.mark.parametrize("ipcp", IPCP, ids=_ipcp_id)
@pytest.mark.parametrize("which", ["edge", "long"])
def test_poisoned_buffers(which, ipcp):
    """The same bytes with the workspace and the outputs pre-filled with 0xFF and with 0x00, and
    from one run to the next: nothing stale is read, nothing relies on zeroed memory."""
    dt = np.complex128 if which == "edge" else np.float32
    A, B = {"edge": gc.edge_pair, "long": gc.long_pair}[which](dt)
    runs = [_run(A, B, 0.3, -2.7, ip=ipcp[0], cp=ipcp[1], fill=f) for f in (0xFF, 0x00, 0xFF, 0x00)]
    gc.assert_equal(runs[0], A, B, 0.3, -2.7, ref=_ref(which, dt, 0.3, -2.7))
    for r in runs[1:]:
        for a, b in zip(r, runs[0]):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ------------------------------------------------------------------ 7. statuses, workspace, timing
def _small():
    return gc.random_pair(70, 33, 500, 400)


def test_size_query_launches_nothing_and_phases():
    from spmm_amd import _lib
    A, B = gc.edge_pair(np.float64)
    c = _Call(A, B, 0.3, -2.7)
    c.h.set_timing(True)
    try:
        assert c.query() == 0 and c.need.value > 0
        after_query = c.h.get_timing()
        assert c.structure() == 0
        after_nnz = c.h.get_timing()
        assert c.values() == 0
        torch.cuda.synchronize()
        after = c.h.get_timing()
    finally:
        c.h.set_timing(False)
    assert all(n == 0 for _, n in after_query.values())
    assert after_nnz["symbolic"][1] == 2 and after_nnz["scan"][1] == 2 and after_nnz["numeric"][1] == 0
    assert after["numeric"][1] == 1
    assert all(n == 0 for k, (_, n) in after.items() if k not in ("symbolic", "scan", "numeric"))
    assert len(_lib.PHASES) == 9 and len(after) == 9
    gc.assert_equal(c.result(), A, B, 0.3, -2.7)


def test_workspace_one_byte_short():
    c = _Call(*_small())
    assert c.query() == 0
    assert c.structure(shrink=1) == INVALID_VALUE
    assert c.structure() == 0
    assert c.values(shrink=1) == INVALID_VALUE
    assert c.values() == 0


def test_null_arguments():
    c = _Call(*_small())
    lib, h = c.lib, c.h.ptr
    a, b, nnz, need = ctypes.byref(c.va), ctypes.byref(c.vb), ctypes.byref(c.nnz), ctypes.byref(c.need)
    assert lib.spg_csrgeam_nnz(None, a, b, None, c.ctype, nnz, need, None) == NOT_INITIALIZED
    assert lib.spg_csrgeam_nnz(h, None, b, None, c.ctype, nnz, need, None) == INVALID_VALUE
    assert lib.spg_csrgeam_nnz(h, a, None, None, c.ctype, nnz, need, None) == INVALID_VALUE
    assert lib.spg_csrgeam_nnz(h, a, b, None, c.ctype, None, need, None) == INVALID_VALUE
    assert lib.spg_csrgeam_nnz(h, a, b, None, c.ctype, nnz, None, None) == INVALID_VALUE
    assert lib.spg_csrgeam_nnz(h, a, b, None, 16, nnz, need, None) == INVALID_VALUE       # bad C_indptr_type
    assert c.query() == 0
    ws = c.buf(c.need.value, torch.uint8)
    wsp = ctypes.c_void_p(ws.data_ptr())
    assert lib.spg_csrgeam_nnz(h, a, b, None, c.ctype, nnz, need, wsp) == INVALID_VALUE   # NULL C_indptr with a workspace
    assert c.structure() == 0
    c.alloc_c()
    al, be, vc, n = ctypes.byref(c.al), ctypes.byref(c.be), ctypes.byref(c.vc), ctypes.c_size_t(c.need.value)
    wsp = ctypes.c_void_p(c.ws.data_ptr())
    assert lib.spg_csrgeam(None, al, a, be, b, vc, n, wsp) == NOT_INITIALIZED
    assert lib.spg_csrgeam(h, None, a, be, b, vc, n, wsp) == INVALID_VALUE
    assert lib.spg_csrgeam(h, al, a, None, b, vc, n, wsp) == INVALID_VALUE
    assert lib.spg_csrgeam(h, al, None, be, b, vc, n, wsp) == INVALID_VALUE
    assert lib.spg_csrgeam(h, al, a, be, None, vc, n, wsp) == INVALID_VALUE
    assert lib.spg_csrgeam(h, al, a, be, b, None, n, wsp) == INVALID_VALUE
    assert lib.spg_csrgeam(h, al, a, be, b, vc, n, None) == INVALID_VALUE
    assert lib.spg_csrgeam(h, al, a, be, b, vc, n, wsp) == 0
    gc.assert_equal(c.result(), *_small(), 1, 1)


@pytest.mark.parametrize("what", ["rows", "cols", "value_type", "indptr_type", "indptr", "indices", "values"])
def test_mismatched_operands(what):
    """B against A: shape, value type, indptr type; a NULL array that is needed."""
    from spmm_amd import _lib
    c = _Call(*_small())
    if what in ("rows", "cols"):
        setattr(c.vb, what, getattr(c.vb, what) + 1)
    elif what == "value_type":
        c.vb.value_type = _lib.SPG_R_32F
    elif what == "indptr_type":
        c.vb.indptr_type = _lib.SPG_INDEX_64I
    else:
        setattr(c.vb, what, None)
    assert c.query() == INVALID_VALUE


@pytest.mark.parametrize("what", ["rows", "cols", "value_type", "indptr_type", "indptr", "indices", "values"])
def test_mismatched_result(what):
    """C against A: shape and value type; a row-pointer type that is no index type; NULL arrays."""
    from spmm_amd import _lib
    c = _Call(*_small())
    assert c.query() == 0 and c.structure() == 0
    c.alloc_c()
    if what in ("rows", "cols"):
        setattr(c.vc, what, getattr(c.vc, what) + 1)
    elif what == "value_type":
        c.vc.value_type = _lib.SPG_R_32F
    elif what == "indptr_type":
        c.vc.indptr_type = 16
    else:
        setattr(c.vc, what, None)
    assert c.values() == INVALID_VALUE


# ------------------------------------------------------------------ 8. special values
@functools.lru_cache(maxsize=None)
def _special_ref(regime, dname, coefs):
    A, B = gc.special_pair(regime, dname)
    return gc.reference(A, B, *coefs), gc.reference_full(A, B, *coefs)


@pytest.mark.parametrize("ipcp", IPCP, ids=_ipcp_id)
@pytest.mark.parametrize("coefs", gc.SPECIAL_COEFS + [(-0.75, 0)], ids=gc.case_id)
@pytest.mark.parametrize("regime", sv.REGIMES)
@pytest.mark.parametrize("dname", list(sv.DTYPES))
def test_special_values(dname, regime, coefs, ipcp):
    """Shares of the reference's components (scipy's values over the union structure), measured
    on the CPU for all four types: NaN <= 2.3 % (cap 10 %); tiny: denormal >= 40 %; huge: inf >= 6 %;
    ints: zero >= 4 %; mixed: NaN >= 0.18 %.  (-0.75, 0) gets the cap alone: huge and tiny do not
    reach their floors there."""
    A, B = gc.special_pair(regime, dname)
    ref, full = _special_ref(regime, dname, coefs)
    sv.check_conditions(regime, full[2], floors=coefs != (-0.75, 0))
    gc.assert_equal(_run(A, B, *coefs, ip=ipcp[0], cp=ipcp[1]), A, B, *coefs, ref=ref)


# ------------------------------------------------------------------ 9. the Python layer
def _parts(m):
    torch.cuda.synchronize()
    return m.indptr.cpu().numpy(), m.indices.cpu().numpy(), m.data.cpu().numpy()


def _dev(S):
    from spmm_amd.sparse import csr_matrix
    return csr_matrix(S, device=DEV)


@pytest.mark.parametrize("dt", DTYPES, ids=_name)
def test_operators(dt):
    from spmm_amd import _lib, cusparse
    from spmm_amd.sparse import coo_matrix, csc_matrix
    A, B = gc.edge_pair(dt)
    dA, dB = _dev(A), _dev(B)
    h = _lib.get_handle(0)
    h.set_timing(True)
    try:
        s, d = dA + dB, dA - dB
        torch.cuda.synchronize()
        launches = h.get_timing()
    finally:
        h.set_timing(False)
    assert launches["numeric"][1] == 2 and launches["symbolic"][1] == 4   # the engine ran, not torch
    assert s._canonical is True and s.shape == A.shape and s.indptr.dtype == torch.int32
    gc.assert_equal(_parts(s), A, B, 1, 1, ref=_ref("edge", dt, 1, 1))
    gc.assert_equal(_parts(d), A, B, 1, -1, ref=_ref("edge", dt, 1, -1))
    gc.assert_equal(_parts(cusparse.csrgeam(dA, dB, 0.3, -2.7)), A, B, 0.3, -2.7, ref=_ref("edge", dt, 0.3, -2.7))
    for got in (-dA, 0 - dA):
        p, j, x = _parts(got)
        assert np.array_equal(p, A.indptr) and np.array_equal(j, A.indices)
        assert np.array_equal(x.view(np.uint8), (-A.data).view(np.uint8))
    for got in (0 + dA, dA - 0):
        assert got is not dA and got.data.data_ptr() != dA.data.data_ptr()
        assert np.array_equal(_parts(got)[2].view(np.uint8), A.data.view(np.uint8))
    mixed = dA + csc_matrix(B, device=DEV)
    assert mixed.format == "csr"
    gc.assert_equal(_parts(mixed), A, B, 1, 1, ref=_ref("edge", dt, 1, 1))
    T = csc_matrix(A, device=DEV) - csc_matrix(B, device=DEV)
    assert T.format == "csc" and T.shape == A.shape
    torch.cuda.synchronize()
    back = sp.csc_matrix((T.data.cpu().numpy(), T.indices.cpu().numpy(), T.indptr.cpu().numpy()),
                         shape=T.shape).tocsr()
    gc.assert_equal((back.indptr, back.indices, back.data), A, B, 1, -1, ref=_ref("edge", dt, 1, -1))
    gc.assert_equal(_parts(dA + coo_matrix(B, device=DEV)), A, B, 1, 1, ref=_ref("edge", dt, 1, 1))


def test_promotion_noncanonical_and_errors():
    from spmm_amd import cusparse
    from spmm_amd.sparse import csr_matrix
    A, B = gc.edge_pair(np.float32)[0], gc.edge_pair(np.float64)[1]
    C = _dev(A) + _dev(B)
    assert C.dtype == np.float64
    gc.assert_equal(_parts(C), A.astype(np.float64), B, 1, 1)
    # a non-canonical operand is summed first: [[1+2, 0, 4]] + [[0, 5, 6]]
    N = csr_matrix((np.array([1.0, 4.0, 2.0]), np.array([0, 2, 0]), np.array([0, 3])), shape=(1, 3), device=DEV)
    P = csr_matrix((np.array([5.0, 6.0]), np.array([1, 2]), np.array([0, 2])), shape=(1, 3), device=DEV)
    S = N + P
    assert S.indices.tolist() == [0, 1, 2] and S.data.tolist() == [3.0, 5.0, 10.0]
    with pytest.raises(ValueError, match="inconsistent shapes"):
        _dev(A) + _dev(sp.csr_matrix((3, 4), dtype=np.float32))
    with pytest.raises(ValueError, match="inconsistent shapes"):
        cusparse.csrgeam2(_dev(A), _dev(sp.csr_matrix((3, 4), dtype=np.float32)))
    with pytest.raises(TypeError, match="unsupported type"):
        cusparse.csrgeam2(_dev(A), A)
    with pytest.raises(NotImplementedError, match="adding a nonzero scalar to a sparse matrix is not supported"):
        _dev(A) + 1.5
    assert _dev(A).__add__(torch.zeros(A.shape, device=DEV)) is NotImplemented
    assert _dev(A).__sub__(np.zeros(A.shape)) is NotImplemented


# ------------------------------------------------------------------ 10. two products compared
def test_two_products_compared_on_the_device():
    """D = spgemm(alg=1) - spgemm(alg=3) on a golden pair: the products' structure, and every
    value +0.0 -- the comparison the numerical_error scripts make through dense arrays."""
    from spmm_amd import cusparse
    from tests.golden_cases import load
    A, B, _, _ = load("config1_n1024_d0.01_f64")
    dA, dB = _dev(A), _dev(B)
    C1 = cusparse.spgemm(dA, dB, alg=1)
    C3 = cusparse.spgemm(dA, dB, alg=3, chunk_fraction=0.3)
    D = C1 - C3
    p, j, x = _parts(D)
    p1, j1, _ = _parts(C1)
    p3, j3, _ = _parts(C3)
    assert D.nnz == C1.nnz == C3.nnz > 0
    assert np.array_equal(p, p1) and np.array_equal(j, j1) and np.array_equal(p, p3) and np.array_equal(j, j3)
    assert not x.view(np.uint8).any()
    assert float(D.data.abs().max()) == 0.0
