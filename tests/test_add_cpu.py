"""A + B, A - B and -A of the device containers on CPU tensors: the torch fallback of
spmm_amd/sparse.py (_geam_torch) against scipy, with the structure and value checks of the GPU
file (tests/geam_cases.py), on the small edge matrix."""
import numpy as np
import pytest
import scipy.sparse as sp

torch = pytest.importorskip("torch")

from tests import geam_cases as gc   # noqa: E402


def _dev(S):
    from spmm_amd.sparse import csr_matrix
    return csr_matrix(S.copy(), device="cpu")


def _parts(C):
    return C.indptr.numpy(), C.indices.numpy(), C.data.numpy()


@pytest.mark.parametrize("dt,coefs", gc.DTYPE_COEFS, ids=gc.case_id)
def test_fallback_matches_scipy(dt, coefs):
    alpha, beta = coefs
    A, B = gc.edge_pair(dt)
    C = _dev(A)._add_sparse(_dev(B), alpha, beta)
    assert C._canonical is True and C.shape == A.shape
    gc.assert_equal(_parts(C), A, B, alpha, beta)


@pytest.mark.parametrize("dt", gc.DTYPES, ids=lambda d: np.dtype(d).name)
def test_operators(dt):
    from spmm_amd.sparse import coo_matrix, csc_matrix
    A, B = gc.edge_pair(dt)
    dA, dB = _dev(A), _dev(B)
    gc.assert_equal(_parts(dA + dB), A, B, 1, 1)
    gc.assert_equal(_parts(dA - dB), A, B, 1, -1)
    for got in (-dA, 0 - dA):
        p, j, x = _parts(got)
        assert np.array_equal(p, A.indptr) and np.array_equal(j, A.indices) and np.array_equal(x, -A.data)
    for got in (0 + dA, dA - 0, dA + 0):
        assert got is not dA and np.array_equal(_parts(got)[2], A.data)
    S = dA + csc_matrix(B, device="cpu")
    assert S.format == "csr"
    gc.assert_equal(_parts(S), A, B, 1, 1)
    T = csc_matrix(A, device="cpu") - csc_matrix(B, device="cpu")
    assert T.format == "csc" and T.shape == A.shape
    want = (A - B).tocsc()
    got = sp.csc_matrix((T.data.numpy(), T.indices.numpy(), T.indptr.numpy()), shape=T.shape).tocsr()
    gc.assert_equal((got.indptr, got.indices, got.data), A, B, 1, -1, ref=want.tocsr())
    gc.assert_equal(_parts(dA + coo_matrix(B, device="cpu")), A, B, 1, 1)
    gc.assert_equal(_parts(coo_matrix(A, device="cpu") - dB), A, B, 1, -1)


def test_self_sum_and_difference():
    A, _ = gc.edge_pair(np.float64)
    dA = _dev(A)
    two = dA + dA
    assert np.array_equal(two.indices.numpy(), A.indices) and np.array_equal(two.data.numpy(), 2 * A.data)
    zero = dA - dA
    assert zero.nnz == A.nnz and not zero.data.numpy().view(np.uint8).any()


def test_promotion_noncanonical_and_errors():
    from spmm_amd.sparse import csr_matrix
    A, B = gc.edge_pair(np.float32)[0], gc.edge_pair(np.float64)[1]
    C = _dev(A) + _dev(B)
    assert C.dtype == np.float64
    gc.assert_equal(_parts(C), A.astype(np.float64), B, 1, 1)
    # a non-canonical operand is summed first: [[1+2, 0, 4]] + [[0, 5, 6]]
    N = csr_matrix((np.array([1.0, 4.0, 2.0]), np.array([0, 2, 0]), np.array([0, 3])), shape=(1, 3), device="cpu",
                   canonical=False)
    P = csr_matrix((np.array([5.0, 6.0]), np.array([1, 2]), np.array([0, 2])), shape=(1, 3), device="cpu", canonical=True)
    S = N + P
    assert S.indices.tolist() == [0, 1, 2] and S.data.tolist() == [3.0, 5.0, 10.0]
    with pytest.raises(ValueError, match="inconsistent shapes"):
        _dev(A) + _dev(sp.csr_matrix((3, 4), dtype=np.float32))
    with pytest.raises(NotImplementedError, match="adding a nonzero scalar to a sparse matrix is not supported"):
        _dev(A) + 1.5
    assert _dev(A)._add(np.zeros(A.shape), False, False) is NotImplemented
    assert _dev(A).__add__(torch.zeros(A.shape)) is NotImplemented
