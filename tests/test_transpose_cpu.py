"""CSR <-> CSC conversion and transposition of the containers on CPU tensors (the torch
conversion: tensors that are not on a GPU never reach spg_csr2csc), against scipy array for array."""
import numpy as np
import pytest
import scipy.sparse as sp

torch = pytest.importorskip("torch")

DTYPES = [np.float32, np.float64, np.complex64, np.complex128]


def _bits(v):
    return np.ascontiguousarray(v).view(np.uint8)


def _same(got, want):
    """got, want: scipy compressed matrices of one format; equal array for array."""
    assert got.shape == want.shape and got.format == want.format
    assert np.array_equal(got.indptr, want.indptr)
    assert np.array_equal(got.indices, want.indices)
    assert got.data.dtype == want.data.dtype
    assert np.array_equal(_bits(got.data), _bits(want.data))


def _matrix(dt, canonical=True):
    rng = np.random.default_rng(3)
    S = sp.random(70, 45, density=0.15, format="csr", random_state=rng).astype(dt)
    if np.dtype(dt).kind == "c":
        S.data = (S.data + 1j * rng.standard_normal(S.nnz)).astype(dt)
    S.sort_indices()
    if not canonical:   # rows reversed in place (unsorted) plus duplicates of every fifth entry
        rows = np.repeat(np.arange(70), np.diff(S.indptr))
        extra = np.arange(0, S.nnz, 5)
        r = np.concatenate([rows, rows[extra]])
        c = np.concatenate([S.indices, S.indices[extra]])
        d = np.concatenate([S.data, (S.data[extra] * 3).astype(dt)])
        order = np.lexsort((-np.arange(r.size), r))
        indptr = np.zeros(71, dtype=np.int32)
        indptr[1:] = np.cumsum(np.bincount(r, minlength=70))
        S = sp.csr_matrix((d[order], c[order].astype(np.int32), indptr), shape=(70, 45))
        assert not S.has_canonical_format
    return S


@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("dt", DTYPES)
def test_tocsc_equals_scipy(dt, canonical):
    from spmm_amd.sparse import csc_matrix, csr_matrix
    S = _matrix(dt, canonical)
    got = csr_matrix(S, device="cpu").tocsc()
    assert isinstance(got, csc_matrix) and got.shape == S.shape
    _same(got.get(), S.tocsc())


def test_tocsc_empty_and_degenerate():
    from spmm_amd.sparse import csr_matrix
    for shape in [(0, 5), (5, 0), (4, 7)]:
        S = sp.csr_matrix(shape, dtype=np.float64)
        _same(csr_matrix(S, device="cpu").tocsc().get(), S.tocsc())


@pytest.mark.parametrize("dt", DTYPES)
def test_T_shares_storage(dt):
    from spmm_amd.sparse import csc_matrix, csr_matrix
    S = _matrix(dt)
    A = csr_matrix(S, device="cpu")
    for T in (A.T, A.transpose()):
        assert isinstance(T, csc_matrix)
        assert T.shape == (S.shape[1], S.shape[0])
        assert T.data.data_ptr() == A.data.data_ptr()
        assert T.indices.data_ptr() == A.indices.data_ptr()
        assert T.indptr.data_ptr() == A.indptr.data_ptr()
        assert T._canonical is True
        _same(T.get(), S.T.tocsc())
    C = A.transpose(copy=True)
    assert C.data.data_ptr() != A.data.data_ptr()
    _same(C.get(), S.T.tocsc())


@pytest.mark.parametrize("dt", DTYPES)
def test_T_tocsr_equals_scipy(dt):
    from spmm_amd.sparse import csr_matrix
    S = _matrix(dt)
    A = csr_matrix(S, device="cpu")
    want = S.T.tocsr()
    _same(A.T.tocsr().get(), want)
    _same(A.transpose_csr().get(), want)
    _same(A.T.transpose().get(), S)            # csc.transpose(): back over the same arrays
    assert A.T.transpose().data.data_ptr() == A.data.data_ptr()


def test_csc_from_arrays_round_trips():
    from spmm_amd.sparse import csc_matrix
    S = _matrix(np.float64).tocsc()
    for arrays in [(S.data, S.indices, S.indptr),
                   tuple(torch.from_numpy(a.copy()) for a in (S.data, S.indices, S.indptr))]:
        C = csc_matrix(arrays, shape=S.shape)
        assert C.shape == S.shape and C.nnz == S.nnz and C.indices.dtype == torch.int32
        _same(C.get(), S)
        _same(C.tocsr().get(), S.tocsr())
    D = csc_matrix(S, "cpu")                   # the positional device stays where it was
    assert D.device.type == "cpu"
    _same(D.get(), S)
    with pytest.raises(ValueError):
        csc_matrix((S.data, S.indices, S.indptr))
    with pytest.raises(ValueError):
        csc_matrix((S.data, S.indices, S.indptr), shape=S.shape[::-1])


def test_transpose_axes_raises():
    from spmm_amd.sparse import csr_matrix
    A = csr_matrix(_matrix(np.float32), device="cpu")
    with pytest.raises(ValueError):
        A.transpose(axes=(1, 0))
    with pytest.raises(ValueError):
        A.T.transpose(axes=(1, 0))
