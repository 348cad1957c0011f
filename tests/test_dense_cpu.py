"""Dense <-> CSR conversion without a GPU: the numpy restatement of the two rules
(tests/dense_cases.py) equals scipy array for array on every case the GPU tests use, and the
torch form the containers take for tensors that are not on a GPU equals scipy too."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests import dense_cases as dc
from tests import special_values as sv

torch = pytest.importorskip("torch")

DNAMES = list(dc.DTYPES)


def _todense_cases(dname):
    yield "duplicates", dc.duplicates_case(dname)
    yield "special", dc.special_case(dname)
    for m, n in dc.TODENSE_SHAPES:
        yield f"lengths-{m}x{n}", dc.lengths_case(dname, m, n)
    yield "empty", sp.csr_matrix((5, 7), dtype=dc.DTYPES[dname])


def _dense_cases(dname):
    for m, n in dc.FROMDENSE_SHAPES:
        yield f"random-{m}x{n}", dc.dense_case(dname, m, n)
    yield "zeros", dc.dense_case(dname, dc.R + 1, dc.S + 1, "zeros")
    yield "full", dc.dense_case(dname, dc.R + 1, dc.S + 1, "full")


def _same_csr(got, want, what):
    p, j, x = got
    assert np.array_equal(np.asarray(p, dtype=np.int64), want.indptr.astype(np.int64)), f"{what}: indptr"
    assert np.array_equal(j, want.indices), f"{what}: indices"
    assert x.dtype == want.data.dtype
    assert np.array_equal(dc.bits(x), dc.bits(want.data)), f"{what}: value bytes"


@pytest.mark.parametrize("dname", DNAMES)
def test_restated_todense_equals_scipy(dname):
    for name, A in _todense_cases(dname):
        with np.errstate(all="ignore"):
            want = A.toarray()
        sv.assert_values_special(dc.ref_todense(A), want, f"{dname} {name}")


@pytest.mark.parametrize("dname", DNAMES)
def test_triple_sums_to_zero_in_stored_order(dname):
    """(1e16, 1.0, -1e16) gives 0.0 only when added in stored order, and a lone -0.0 arrives as
    +0.0: the cases do tell a wrong order from the right one."""
    D = dc.duplicates_case(dname).toarray()
    for cell in dc.TRIPLE_CELLS:
        assert D[cell] == 0 and not np.signbit(D[cell].real), cell
    dt = dc.DTYPES[dname]
    assert dt(1e16) + dt(-1e16) + dt(1.0) == 1
    Z = sp.csr_matrix((np.array([-0.0], dtype=dt), np.array([0], dtype=np.int32), np.array([0, 1], dtype=np.int32)),
                      shape=(1, 1))
    assert not np.signbit(Z.toarray()[0, 0].real) and not np.signbit(dc.ref_todense(Z)[0, 0].real)


@pytest.mark.parametrize("dname", DNAMES)
def test_restated_fromdense_equals_scipy(dname):
    for name, D in _dense_cases(dname):
        _same_csr(dc.ref_fromdense(D), sp.csr_matrix(D), f"{dname} {name}")
        pt, jt, xt = dc.ref_fromdense(D.T)         # CSC: the CSR form of the transpose
        _same_csr((pt, jt, xt), sp.csc_matrix(D), f"{dname} {name} csc")
    D = dc.dense_case(dname, dc.R + 1, dc.S + 1)
    kept = dc.keep_mask(D)
    comps = np.ascontiguousarray(D).view(dc.real_dtype(D.dtype)).reshape(D.shape + (-1,))
    tiny = np.finfo(comps.dtype).tiny
    assert (np.isnan(comps).any(-1) & kept).any() and ((np.abs(comps) > 0) & (np.abs(comps) < tiny)).any()
    assert (np.signbit(comps).any(-1) & ~kept).any()           # a -0.0 that is dropped


@pytest.mark.parametrize("dname", DNAMES)
def test_torch_todense_equals_scipy(dname):
    from spmm_amd.sparse import coo_matrix, csc_matrix, csr_matrix
    for name, A in _todense_cases(dname):
        with np.errstate(all="ignore"):
            want = A.toarray()
        dA = csr_matrix((A.data, A.indices, A.indptr), shape=A.shape, device="cpu")
        got = dA.todense()
        assert isinstance(got, torch.Tensor) and got.is_contiguous() and tuple(got.shape) == A.shape
        sv.assert_values_special(got.numpy(), want, f"{dname} {name}")
    A = dc.duplicates_case(dname)
    with np.errstate(all="ignore"):
        want = A.toarray()
    dA = csr_matrix((A.data, A.indices, A.indptr), shape=A.shape, device="cpu")
    f = dA.todense(order="F")
    assert f.stride(0) == 1 and np.array_equal(dc.bits(f.numpy()), dc.bits(want))
    out = torch.full((A.shape[0], A.shape[1] + 3), 7, dtype=f.dtype)[:, :A.shape[1]]
    assert dA.todense(out=out) is out and np.array_equal(dc.bits(out.numpy()), dc.bits(want))
    # the same arrays read as CSC are the transpose
    dC = csc_matrix((A.data, A.indices, A.indptr), shape=A.shape[::-1], device="cpu")
    assert np.array_equal(dc.bits(dC.todense().numpy()), dc.bits(want.T))
    # COO, entries in a shuffled order: per element still the stored order
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    perm = np.random.default_rng(3).permutation(A.nnz)
    C = sp.coo_matrix((A.data[perm], (rows[perm], A.indices[perm])), shape=A.shape)
    dO = coo_matrix((torch.from_numpy(C.data), (C.row, C.col)), shape=A.shape, device="cpu")
    with np.errstate(all="ignore"):
        sv.assert_values_special(dO.todense().numpy(), C.toarray(), f"{dname} coo")
    with pytest.raises(ValueError):
        dA.todense(order="K")
    with pytest.raises(ValueError):
        dA.todense(out=torch.zeros(2, 2, dtype=f.dtype))
    assert isinstance(dA.toarray(), np.ndarray)     # toarray() keeps returning numpy


@pytest.mark.parametrize("dname", DNAMES)
def test_torch_dense_constructor_equals_scipy(dname):
    from spmm_amd.sparse import csc_matrix, csr_matrix
    for name, D in _dense_cases(dname):
        for arg in (torch.from_numpy(D.copy()), D, torch.from_numpy(np.asfortranarray(D)).t().contiguous().t()):
            c = csr_matrix(arg, device="cpu")
            assert c.shape == D.shape and c._canonical is True and c.indices.dtype == torch.int32
            _same_csr((c.indptr.numpy(), c.indices.numpy(), c.data.numpy()), sp.csr_matrix(D), f"{dname} {name}")
        c = csc_matrix(torch.from_numpy(D.copy()), device="cpu")
        assert c.shape == D.shape and c._canonical is True
        _same_csr((c.indptr.numpy(), c.indices.numpy(), c.data.numpy()), sp.csc_matrix(D), f"{dname} {name} csc")
    with pytest.raises(ValueError):
        csr_matrix(torch.zeros(3), device="cpu")
    with pytest.raises(TypeError):
        csr_matrix(torch.zeros((2, 2), dtype=torch.int32), device="cpu")
    with pytest.raises(TypeError):
        csr_matrix("not a matrix")
    with pytest.raises(TypeError):
        csc_matrix("not a matrix")


def test_cusparse_names_and_cpu_operands():
    from spmm_amd import cusparse
    from spmm_amd.sparse import csr_matrix
    for name in ("csr2dense", "csc2dense", "dense2csr", "dense2csc", "denseToSparse", "sparseToDense"):
        assert isinstance(cusparse.check_availability(name), bool)
    A = dc.lengths_case("f64", 1, 63)
    dA = csr_matrix((A.data, A.indices, A.indptr), shape=A.shape, device="cpu")
    for call in (lambda: cusparse.csr2dense(dA), lambda: cusparse.sparseToDense(dA),
                 lambda: cusparse.dense2csr(torch.zeros(2, 2, dtype=torch.float64)),
                 lambda: cusparse.dense2csc(torch.zeros(2, 2, dtype=torch.float64)),
                 lambda: cusparse.denseToSparse(torch.zeros(2, 2, dtype=torch.float64))):
        with pytest.raises(RuntimeError):
            call()


def test_int32_overflow_is_retried_with_int64(monkeypatch):
    """The binding's side of SPG_STATUS_OVERFLOW, against a stand-in library (2**31 kept elements
    need a D of 8 GiB and more): int32 row pointers first; when the engine reports that nnz does
    not fit, the structure call is repeated with an int64 array and the fill uses that one."""
    from spmm_amd import _lib, cusparse
    calls = []

    class Lib:
        def spg_dense2csr_nnz(self, h, vd, indptr, itype, nnz, need, ws):
            calls.append(("nnz", itype, ws is not None))
            if ws is None:
                need._obj.value = 64
                return 0
            if itype == _lib.SPG_INDEX_32I:
                nnz._obj.value = 2 ** 31 + 5          # reported even though it does not fit
                return _lib.STATUS_OVERFLOW
            nnz._obj.value = 0
            return 0

        def spg_dense2csr(self, h, vd, vc, nbytes, ws):
            calls.append(("fill", vc._obj.indptr_type, vc._obj.nnz))
            return 0

    class Handle:
        lib, ptr = Lib(), None
    monkeypatch.setattr(cusparse, "_handle_on", lambda dev: Handle())
    data, indices, indptr = cusparse._dense2csr_arrays(torch.zeros(3, 4, dtype=torch.float64))
    assert calls == [("nnz", 32, False), ("nnz", 32, True), ("nnz", 64, True), ("fill", 64, 0)]
    assert indptr.dtype == torch.int64 and indptr.numel() == 4 and data.numel() == indices.numel() == 0
