"""The cached canonical flag on CPU tensors, where the torch forms serve: every operation of
tests/canonical_flag_cases.OPS on every source, entered every way, under that module's rule -- the
flag may be unknown but may not lie, ``has_canonical_format`` resolves it to the truth recomputed
from the result's arrays, and the values are scipy's.  tests/test_gpu_canonical_flag.py runs the
same list on device tensors.
"""
import numpy as np
import pytest
import scipy.sparse as sp

torch = pytest.importorskip("torch")

from tests import canonical_flag_cases as fc          # noqa: E402
from tests import validate_cases as vc                # noqa: E402
from spmm_amd.sparse import csc_matrix, csr_matrix    # noqa: E402

CPU = "cpu"


# ------------------------------------------------------------------ the sources are what they say
@pytest.mark.parametrize("dt", [np.float64, np.complex64], ids=["f64", "c64"])
@pytest.mark.parametrize("fmt", ["csr", "csc"])
def test_sources(fmt, dt):
    n_major = fc.M if fmt == "csr" else fc.N
    got = {}
    for kind in fc.KINDS:
        S = fc.source(kind, fmt, dt)
        assert S.shape == (fc.M, fc.N) and S.dtype == dt and S.indices.dtype == np.int32
        p, j, x = S.indptr, S.indices, S.data
        n_minor = fc.N if fmt == "csr" else fc.M
        status = vc.canon_status(p, j, n_minor, len(j))
        fresh = (sp.csr_matrix if fmt == "csr" else sp.csc_matrix)((x.copy(), j.copy(), p.copy()), shape=S.shape)
        assert (status == 1) == bool(fresh.has_canonical_format) and status != -1
        lens = np.diff(p)
        assert all(lens[i] == 0 for i in (0, 5, 6, n_major - 2)) and lens[n_major - 1] >= 4
        assert np.all(np.abs(x.real) <= 8) and np.all(np.abs(x.imag) <= 8) and np.all(x.real == np.round(x.real))
        pairs = [(i, q) for i in range(n_major) for q in range(p[i] + 1, p[i + 1]) if j[q] <= j[q - 1]]
        dups = [(i, q) for i, q in pairs if j[q] == j[q - 1]]
        got[kind] = (status, sorted({i for i, _ in pairs}), dups)
        if kind not in ("MIX", "ZTW"):
            assert np.count_nonzero(x) == x.size
    assert got["CAN"] == (1, [], [])
    assert got["UNS"][:2] == (0, [2, 17, n_major - 1]) and got["UNS"][2] == []
    assert got["DUP"][:2] == (0, [9, 26]) and [i for i, _ in got["DUP"][2]] == [9, 26]
    assert got["MIX"][:2] == (0, [2, 9, 17, 26, n_major - 1]) and [i for i, _ in got["MIX"][2]] == [9, 26]
    assert got["ZTW"][:2] == (0, [9, 26]) and [i for i, _ in got["ZTW"][2]] == [9, 26]
    S = fc.source("MIX", fmt, dt)
    (_, q9), (_, q26) = got["MIX"][2]
    assert S.data[q9] + S.data[q9 - 1] == 0 and S.data[q9] != 0          # a pair that sums to an exact zero
    assert S.data[q26 - 1] == 0 and S.data[q26] != 0                     # a stored zero beside its twin
    S = fc.source("ZTW", fmt, dt)
    (_, q9), (_, q26) = got["ZTW"][2]
    assert np.flatnonzero(S.data == 0).tolist() == [q9, q26 - 1]         # the zero after its twin, and before it
    S.eliminate_zeros()
    assert S.has_canonical_format                                        # only the zero twins stood in the way


def test_entries_start_with_the_flag_they_should():
    for kind in fc.KINDS:
        truth = kind == "CAN"
        S = fc.source(kind)
        assert fc.enter(S, "scipy", CPU)._canonical is truth
        assert fc.enter(S, "none", CPU)._canonical is None
        assert fc.enter(S, "flag", CPU)._canonical is truth
        C = fc.source(kind, "csc")
        assert fc.enter(C, "scipy", CPU)._canonical is (True if truth else None)
        assert fc.enter(C, "flag", CPU)._canonical is truth
        for entry in fc.ENTRIES:
            for A in (fc.enter(S, entry, CPU), fc.enter(C, entry, CPU)):
                assert isinstance(A, (csr_matrix, csc_matrix)) and A.device.type == "cpu"
                assert np.array_equal(A.toarray(), fc.source(kind, A.format).toarray())


# ------------------------------------------------------------------ the list
@pytest.mark.parametrize("op", fc.OPS, ids=fc.OP_IDS)
def test_flag_never_lies_f64(op):
    failures = fc.sweep(op, CPU, np.float64)
    assert not failures, "\n" + "\n".join(failures)


@pytest.mark.parametrize("op", fc.OPS, ids=fc.OP_IDS)
def test_flag_never_lies_c64(op):
    """One pass over the list with complex64 values, every source entered with the flag unknown."""
    failures = fc.sweep(op, CPU, np.complex64, entries=("none",))
    assert not failures, "\n" + "\n".join(failures)


# ------------------------------------------------------------------ the three predictions, by name
def test_unknown_flag_resolves_on_cpu_tensors():
    S = fc.source("DUP")
    A = csr_matrix((S.data, S.indices, S.indptr), shape=S.shape, device=CPU)
    assert A._canonical is None and A.has_canonical_format is False
    A = csr_matrix((S.data, S.indices, S.indptr), shape=S.shape, device=CPU)
    A.sum_duplicates()
    assert A._canonical is True and fc.truth_of(A)
    A = csr_matrix(fc.source("CAN"), device=CPU)[:, [1, 0, 1]]
    assert A._canonical is None
    A.sum_duplicates()
    assert A._canonical is True and fc.truth_of(A)
    want = fc.source("CAN")[:, [1, 0, 1]]
    assert np.array_equal(A.toarray(), want.toarray())


def test_sort_indices_keeps_duplicates():
    """2 x 3, four stored entries, two of them duplicates: four afterwards, as scipy and csrsort."""
    data, indices, indptr = np.array([1.0, 2.0, 3.0, 4.0]), np.array([2, 0, 2, 1], dtype=np.int32), np.array([0, 3, 4])
    A = csr_matrix((data, indices, indptr), shape=(2, 3), device=CPU)
    S = sp.csr_matrix((data.copy(), indices.copy(), indptr.copy()), shape=(2, 3))
    A.sort_indices()
    S.sort_indices()
    assert A.nnz == S.nnz == 4 and A._canonical is None
    assert A.indices.tolist() == [0, 2, 2, 1] and A.data.tolist() == [2.0, 1.0, 3.0, 4.0]      # stable
    assert A.has_canonical_format is False
    T = csr_matrix(fc.source("CAN"), device=CPU)
    before = T.indices.data_ptr()
    T.sort_indices()
    assert T._canonical is True and T.indices.data_ptr() == before                          # True stays True, untouched


def test_false_does_not_travel_to_a_canonical_result():
    for kind in ("UNS", "DUP", "MIX"):
        S = fc.source(kind)
        A = csr_matrix(S, device=CPU)
        assert A._canonical is False
        good = [i for i in range(fc.M) if i not in fc.noncanonical_segments(S)]
        sub = A[good]
        assert sub._canonical is None and fc.truth_of(sub) and sub.has_canonical_format is True
    Z = csr_matrix(fc.source("ZTW"), device=CPU)
    assert Z._canonical is False
    Z.eliminate_zeros()
    assert Z._canonical is None and fc.truth_of(Z) and Z.has_canonical_format is True
    D = csr_matrix(fc.source("DUP"), device=CPU)        # nothing to drop: the structure, and the flag, stay
    D.eliminate_zeros()
    assert D._canonical is False and not fc.truth_of(D)
