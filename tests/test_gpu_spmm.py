"""SpMM parity (CSR x dense matrix: the dense half of others/spmm/spMM.py and
others/spmm/diff_matrix_size.py; cupyx.cusparse.spmm, modify_src/cupy-src/cupyx/cusparse.py:
1440-1513), through the C ABI (spg_spmm).

Bar: CSR A @ B bit-exact against scipy's csr_matvecs on the host, in both dense orders, with
leading dimensions and misaligned bases; C = alpha*A B + beta*C bit-exact against the same
elementwise expression in numpy; CSC / COO operands and op(A) = A^T within a stated tolerance
(they reach CSR through a conversion, and scipy sums those in a different order):
|C - C_ref| <= 1e-12 (f64), 1e-4 (f32) relative to max(|A| |X|).
"""
import ctypes
import functools

import numpy as np
import pytest
import scipy.sparse as sp

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64, np.complex64, np.complex128]
M, K = 600, 500


def _bits(v):
    return np.ascontiguousarray(v).view(np.uint8)


def _values(rng, shape, dt):
    v = rng.standard_normal(shape)
    if np.dtype(dt).kind == "c":
        v = v + 1j * rng.standard_normal(shape)
    return v.astype(dt)


@functools.lru_cache(maxsize=None)
def _edge_matrix(dt):
    """600 x 500 canonical CSR: rows of 0, 1, 63, 64, 65 and 200 entries (the batch-of-64
    boundary and a multi-batch row), a run of empty rows, otherwise a random fill."""
    rng = np.random.default_rng(11)
    lens = rng.integers(0, 40, size=M)
    lens[:6] = [0, 1, 63, 64, 65, 200]
    lens[100:171] = 0
    lens[M - 1] = 130
    indptr = np.zeros(M + 1, dtype=np.int32)
    indptr[1:] = np.cumsum(lens)
    indices = np.concatenate([np.sort(rng.choice(K, size=int(n), replace=False)) for n in lens]).astype(np.int32)
    A = sp.csr_matrix((_values(rng, indices.size, dt), indices, indptr), shape=(M, K))
    assert A.has_canonical_format
    return A


@functools.lru_cache(maxsize=None)
def _edge_device(dt):
    from spmm_amd.sparse import csr_matrix
    return csr_matrix(_edge_matrix(dt), device="cuda:0")


@functools.lru_cache(maxsize=None)
def _edge_case(dt, n):
    """(B on the host, scipy's A @ B) -- computed once, shared, never written."""
    B = _values(np.random.default_rng(100 + n), (K, n), dt)
    want = _edge_matrix(dt) @ B
    B.setflags(write=False)
    want.setflags(write=False)
    return B, want


def _host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


@pytest.mark.parametrize("n", [1, 2, 3, 17, 64, 65, 130, 257, 513])
@pytest.mark.parametrize("dt", DTYPES)
def test_spmm_row_major_bitexact(dt, n):
    """Packed-row widths, a partial last strip, more than one strip for every V."""
    from spmm_amd import cusparse
    B, want = _edge_case(dt, n)
    c = cusparse.spmm(_edge_device(dt), torch.from_numpy(B.copy()).cuda())
    assert c.shape == (M, n) and c.is_contiguous()
    got = _host(c)
    assert got.dtype == want.dtype
    assert np.array_equal(_bits(got), _bits(want))


@pytest.mark.parametrize("n", [1, 3, 17, 65])
@pytest.mark.parametrize("dt", DTYPES)
def test_spmm_col_major_bitexact(dt, n):
    from spmm_amd import cusparse
    B, want = _edge_case(dt, n)
    Bd = torch.from_numpy(B.copy()).cuda().t().contiguous().t()
    c = torch.zeros((n, M), dtype=Bd.dtype, device="cuda:0").t()
    out = cusparse.spmm(_edge_device(dt), Bd, c=c)
    assert out is c
    assert np.array_equal(_bits(_host(c)), _bits(want))
    # without c the result takes b's order
    out = cusparse.spmm(_edge_device(dt), Bd)
    if n > 1:
        assert out.stride() == (1, M)
    assert np.array_equal(_bits(_host(out)), _bits(want))


@pytest.mark.parametrize("off,width", [(1, 7), (4, 14)])
@pytest.mark.parametrize("n", [17, 130])
@pytest.mark.parametrize("dt", DTYPES)
def test_spmm_leading_dimensions_and_alignment(dt, n, off, width):
    """B and c are column slices of wider row-major tensors: ld != n, and with off = 1 a base
    that is not 16-byte aligned (the scalar-width path); with off = 4 and a parent width that is
    a multiple of 4 the fp32 rows stay 16-byte aligned (16-byte accesses with ld != n).  The
    parent's columns outside c keep their sentinel."""
    from spmm_amd import cusparse
    B, want = _edge_case(dt, n)
    tdt = torch.from_numpy(B[:1].copy()).dtype
    big = torch.zeros((K, n + width), dtype=tdt, device="cuda:0")
    big[:, off:off + n] = torch.from_numpy(B.copy()).cuda()
    Bd = big[:, off:off + n]
    parent = torch.full((M, n + width), 7.5, dtype=tdt, device="cuda:0")
    c = parent[:, off:off + n]
    out = cusparse.spmm(_edge_device(dt), Bd, c=c)
    assert out is c
    got = _host(parent)
    assert np.array_equal(_bits(got[:, off:off + n]), _bits(want))
    assert np.all(got[:, :off] == 7.5) and np.all(got[:, off + n:] == 7.5)


@functools.lru_cache(maxsize=None)
def _alpha_beta_case():
    rng = np.random.default_rng(6)
    A = sp.random(2000, 2000, density=0.01, format="csr", random_state=rng)
    A.sort_indices()
    B = rng.standard_normal((2000, 17))
    c0 = rng.standard_normal((2000, 17))
    return A, B, c0, A @ B


@pytest.mark.parametrize("ip", ["int32", "int64"])
def test_spmm_alpha_beta(ip):
    from spmm_amd import cusparse
    from spmm_amd.sparse import csr_matrix
    A, B, c0, AB = _alpha_beta_case()
    dA = csr_matrix(A, device="cuda:0")
    dA.indptr = dA.indptr.to(getattr(torch, ip))
    c = torch.from_numpy(c0.copy()).cuda()
    cusparse.spmm(dA, torch.from_numpy(B.copy()).cuda(), c=c, alpha=-1.5, beta=0.25)
    want = np.float64(-1.5) * AB + np.float64(0.25) * c0
    assert np.array_equal(_bits(_host(c)), _bits(want))


@pytest.mark.parametrize("colmajor", [False, True])
def test_spmm_beta_zero_does_not_read_c(colmajor):
    from spmm_amd import cusparse
    from spmm_amd.sparse import csr_matrix
    A, B, _, AB = _alpha_beta_case()
    Bd = torch.from_numpy(B.copy()).cuda()
    c = torch.full((2000, 17), float("nan"), dtype=torch.float64, device="cuda:0")
    if colmajor:
        Bd = Bd.t().contiguous().t()
        c = torch.full((17, 2000), float("nan"), dtype=torch.float64, device="cuda:0").t()
    cusparse.spmm(csr_matrix(A, device="cuda:0"), Bd, c=c, beta=0)
    got = _host(c)
    assert np.isfinite(got).all()
    assert np.array_equal(_bits(got), _bits(AB))


def test_spmm_dense_offsets_are_64_bit():
    """ld = 2**30 + 8: the last B row starts past 2**31 elements."""
    from spmm_amd import cusparse
    from spmm_amd.sparse import csr_matrix
    free, _ = torch.cuda.mem_get_info()
    if free < 12 * 2 ** 30:
        pytest.skip(f"needs 12 GiB of free device memory for an 8 GiB view, {free / 2 ** 30:.1f} GiB free")
    rng = np.random.default_rng(9)
    A = sp.csr_matrix(np.array([[0, 0, 1.5], [2.0, 0, -3.0], [0, 0, 0], [0.5, 4.0, 7.0]], dtype=np.float32))
    B = rng.standard_normal((3, 64)).astype(np.float32)
    ld = 2 ** 30 + 8
    buf = torch.empty(2 * ld + 64, dtype=torch.float32, device="cuda:0")
    Bd = buf.as_strided((3, 64), (ld, 1))
    Bd.copy_(torch.from_numpy(B).cuda())
    c = cusparse.spmm(csr_matrix(A, device="cuda:0"), Bd)
    got = _host(c)
    del Bd, buf
    torch.cuda.empty_cache()
    assert np.array_equal(_bits(got), _bits(A @ B))


def test_spmm_dispatch_and_formats():
    from spmm_amd import cusparse
    from spmm_amd.sparse import coo_matrix, csc_matrix, csr_matrix
    rng = np.random.default_rng(7)
    A = sp.random(700, 400, density=0.02, format="csr", random_state=rng)
    A.data = rng.standard_normal(A.nnz)
    A.sort_indices()
    X = rng.standard_normal((400, 33))
    Xt = rng.standard_normal((700, 5))
    dA = csr_matrix(A, device="cuda:0")
    want = A @ X
    # numpy 2-D right operand is uploaded; @ and .dot dispatch to spmm; row-major in, row-major out
    for got in (dA @ X, dA.dot(X), dA @ torch.from_numpy(X).cuda()):
        assert got.is_contiguous()
        assert np.array_equal(_bits(_host(got)), _bits(want))
    # transb is a view: X^T stored row-major is X column-major
    XT = torch.from_numpy(np.ascontiguousarray(X.T)).cuda()
    got = cusparse.spmm(dA, XT, transb=True)
    assert got.shape == (700, 33)
    assert np.array_equal(_bits(_host(got)), _bits(want))
    for dt, rel in ((np.float64, 1e-12), (np.float32, 1e-4)):
        Ad, Xd, Xtd = A.astype(dt), X.astype(dt), Xt.astype(dt)
        tol = rel * float((abs(Ad) @ np.abs(Xd)).max())
        ref = (Ad @ Xd).astype(np.float64)
        xd = torch.from_numpy(Xd).cuda()
        for Mx in (csc_matrix(Ad, device="cuda:0"), coo_matrix(Ad, device="cuda:0")):
            got = Mx @ xd
            assert got.is_contiguous()
            np.testing.assert_allclose(_host(got).astype(np.float64), ref, rtol=0, atol=tol)
        got = cusparse.spmm(csr_matrix(Ad, device="cuda:0"), torch.from_numpy(Xtd).cuda(), transa=True)
        tol_t = rel * float((abs(Ad.T) @ np.abs(Xtd)).max())
        np.testing.assert_allclose(_host(got).astype(np.float64), (Ad.T @ Xtd).astype(np.float64), rtol=0, atol=tol_t)


def test_spmm_reference_errors():
    """cusparse.py:1474-1492: TypeError for an unsupported operand, ValueError for a shape
    mismatch; nnz == 0 gives zeros.  The C ABI rejects a mixed-order pair and a short ld
    without launching."""
    from spmm_amd import _lib, cusparse
    from spmm_amd.sparse import csr_matrix
    A = sp.random(30, 20, density=0.2, format="csr", random_state=1)
    dA = csr_matrix(A, device="cuda:0")
    ok = torch.zeros((20, 4), dtype=torch.float64, device="cuda:0")
    with pytest.raises(TypeError):
        cusparse.spmm(A, ok)
    with pytest.raises(ValueError):
        cusparse.spmm(dA, torch.zeros((21, 4), dtype=torch.float64, device="cuda:0"))
    with pytest.raises(ValueError):
        cusparse.spmm(dA, ok, c=torch.zeros((30, 5), dtype=torch.float64, device="cuda:0"))
    with pytest.raises(TypeError):
        cusparse.spmm(dA, ok, c=torch.zeros((30, 4), dtype=torch.float32, device="cuda:0"))
    with pytest.raises(ValueError):
        dA @ torch.zeros((20, 4, 2), dtype=torch.float64, device="cuda:0")
    Z = csr_matrix(sp.csr_matrix((30, 20)), device="cuda:0")
    c = torch.ones((30, 4), dtype=torch.float64, device="cuda:0")
    assert torch.count_nonzero(cusparse.spmm(Z, torch.ones((20, 4), dtype=torch.float64, device="cuda:0"), c=c)) == 0

    h = cusparse._handle_for(dA)
    va = cusparse._csr_view(dA)
    cbuf = torch.zeros((30, 4), dtype=torch.float64, device="cuda:0")
    one, zero = ctypes.c_double(1.0), ctypes.c_double(0.0)

    def call(vb, vc):
        return h.lib.spg_spmm(h.ptr, ctypes.byref(va), ctypes.byref(vb), ctypes.byref(one), ctypes.byref(zero),
                              ctypes.byref(vc))
    row_b = _lib.SpgDense(20, 4, 4, ok.data_ptr(), _lib.SPG_ORDER_ROW, _lib.SPG_R_64F)
    col_c = _lib.SpgDense(30, 4, 30, cbuf.data_ptr(), _lib.SPG_ORDER_COL, _lib.SPG_R_64F)
    short_b = _lib.SpgDense(20, 4, 3, ok.data_ptr(), _lib.SPG_ORDER_ROW, _lib.SPG_R_64F)
    row_c = _lib.SpgDense(30, 4, 4, cbuf.data_ptr(), _lib.SPG_ORDER_ROW, _lib.SPG_R_64F)
    h.set_timing(True)
    try:
        assert call(row_b, col_c) == _lib.STATUS_NOT_SUPPORTED
        assert call(short_b, row_c) == 3   # SPG_STATUS_INVALID_VALUE
        assert all(n == 0 for _, n in h.get_timing().values())
    finally:
        h.set_timing(False)
    assert torch.count_nonzero(cbuf) == 0


def test_spmm_is_timed_under_the_spmv_phase():
    from spmm_amd import cusparse
    dA = _edge_device(np.float64)
    B, want = _edge_case(np.float64, 17)
    Bd = torch.from_numpy(B.copy()).cuda()
    h = cusparse._handle_for(dA)
    h.set_timing(True)
    try:
        c = cusparse.spmm(dA, Bd)
        t = h.get_timing()
    finally:
        h.set_timing(False)
    assert t["spmv"][1] == 1
    assert all(n == 0 for name, (_, n) in t.items() if name != "spmv")
    assert np.array_equal(_bits(_host(c)), _bits(want))
