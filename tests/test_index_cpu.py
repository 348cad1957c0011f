"""Submatrix extraction on CPU tensors: index_cases.restate (the rule of spg_csr_extract,
include/spgemm.h) against scipy, and the containers' __getitem__ -- the torch form of the same
rule, sparse._extract_torch -- against restate, array for array.

scipy comparison: array for array wherever the column selection has no repeat; with repeats scipy
orders them by np.argsort(idx), which is not stable, so a canonical A is compared after
sort_indices() on both sides and a non-canonical A as per-row multisets of (column, value bits).
"""
import numpy as np
import pytest
import scipy.sparse as sp

torch = pytest.importorskip("torch")

from tests import index_cases as ic          # noqa: E402
from tests import special_values as sv      # noqa: E402
from spmm_amd.sparse import csc_matrix, csr_matrix   # noqa: E402


def _name(dt):
    return np.dtype(dt).name


def _parts(M):
    return M.indptr.cpu().numpy(), M.indices.cpu().numpy(), M.data.cpu().numpy()


def _scipy(S, rs, cs):
    m, n = S.shape
    return S[ic.py_key(rs, m)][:, ic.py_key(cs, n)]


def _row_multisets(p, j, x):
    b = ic.bits(x).reshape(len(j), 2 if np.asarray(x).dtype.kind == "c" else 1)
    return [sorted((int(j[e]), tuple(int(w) for w in b[e])) for e in range(p[r], p[r + 1])) for r in range(len(p) - 1)]


# ------------------------------------------------------------------ 1. the rule against scipy
@pytest.mark.parametrize("which", ["cases", "random_cases"])
def test_restate_against_scipy(which):
    compared = {"exact": 0, "sorted": 0, "multiset": 0}
    for cid, name, rs, cs in getattr(ic, which)():
        S = ic.MATRICES[name]()
        want = ic.expected(S, rs, cs)
        R = _scipy(S, rs, cs)
        assert R.shape == (ic.count_of(rs, S.shape[0]), ic.count_of(cs, S.shape[1])), cid
        if not ic.has_repeat(cs):
            ic.same_arrays(want, (R.indptr, R.indices, R.data), cid)
            compared["exact"] += 1
        elif S.has_canonical_format:
            W = sp.csr_matrix(want[::-1], shape=R.shape)
            W.sort_indices()
            R.sort_indices()
            ic.same_arrays((W.indptr, W.indices, W.data), (R.indptr, R.indices, R.data), cid)
            compared["sorted"] += 1
        else:
            assert np.array_equal(want[0], R.indptr), cid
            assert _row_multisets(*want) == _row_multisets(R.indptr, R.indices, R.data), cid
            compared["multiset"] += 1
    assert all(v > 0 for v in compared.values()), compared


# ------------------------------------------------------------------ 2. the containers against the rule
@pytest.mark.parametrize("dt", ic.DTYPES, ids=_name)
@pytest.mark.parametrize("name", list(ic.MATRICES))
def test_csr_getitem(name, dt):
    S = ic.MATRICES[name](dt)
    A = csr_matrix(S, device="cpu")
    m, n = S.shape
    for cid, cname, rs, cs in ic.cases():
        if cname != name:
            continue
        C = A[ic.py_key(rs, m), ic.py_key(cs, n)] if not (rs and cs and rs[0] == cs[0] == "list") else \
            A[ic.py_key(rs, m)][:, ic.py_key(cs, n)]
        assert isinstance(C, csr_matrix) and C.shape == (ic.count_of(rs, m), ic.count_of(cs, n)), cid
        assert C.dtype == np.dtype(dt) and C.indptr.numel() == C.shape[0] + 1
        ic.same_arrays(ic.expected(S, rs, cs), _parts(C), cid)


@pytest.mark.parametrize("dt", ic.DTYPES, ids=_name)
@pytest.mark.parametrize("name", list(ic.MATRICES))
def test_csc_getitem(name, dt):
    """A CSC matrix is the CSR extraction of its transpose with the selections swapped."""
    S = ic.MATRICES[name](dt)
    T = sp.csr_matrix((S.data, S.indices, S.indptr), shape=S.shape)       # the arrays of A^T in CSC
    A = csc_matrix((S.data, S.indices, S.indptr), shape=S.shape[::-1], device="cpu")
    m, n = S.shape
    for cid, cname, rs, cs in ic.cases()[::3]:
        if cname != name:
            continue
        C = A[ic.py_key(cs, n)][:, ic.py_key(rs, m)]
        assert isinstance(C, csc_matrix) and C.shape == (ic.count_of(cs, n), ic.count_of(rs, m)), cid
        ic.same_arrays(ic.expected(T, rs, cs), _parts(C), cid)


def test_keys_name_the_same_submatrix():
    S = ic.small()
    A = csr_matrix(S, device="cpu")
    rows, cols = [5, 0, 22, 5], [3, 36, 1]
    want = ic.expected(S, ("list", rows), ("list", cols))
    for C in (A[rows][:, cols], A[np.ix_(rows, cols)], A[np.array(rows)[:, None], torch.tensor(cols)[None, :]],
              A[torch.tensor(rows)][:, np.array(cols, dtype=np.int32)]):
        ic.same_arrays(want, _parts(C))
    ic.same_arrays(ic.expected(S, ("list", rows), ("range", 4, 1, 16)), _parts(A[rows, 4:20]))
    ic.same_arrays(ic.expected(S, ("range", 2, 1, 7), ("list", cols)), _parts(A[2:9, cols]))
    ic.same_arrays(ic.expected(S, ("list", rows), None), _parts(A[rows]))
    ic.same_arrays(ic.expected(S, None, ("range", 10, 1, 27)), _parts(A[..., 10:]))


def test_negative_steps_indices_and_masks():
    S = ic.small()
    A = csr_matrix(S, device="cpu")
    m, n = S.shape
    ic.same_arrays(ic.expected(S, ("range", m - 1, -1, m), ("range", n - 1, -2, (n + 1) // 2)), _parts(A[::-1, ::-2]))
    ic.same_arrays(ic.expected(S, ("range", m - 3, 1, 2), ("range", n - 5, 1, 3)), _parts(A[-3:-1, -5:-2]))
    ic.same_arrays(ic.expected(S, ("range", 20, -4, 5), None), _parts(A[20:1:-4]))
    ic.same_arrays(ic.expected(S, ("list", [m - 1, 0, m - 2]), ("list", [n - 1, n - 37])),
                   _parts(A[[-1, 0, -2]][:, [-1, -37]]))
    mask_r = np.zeros(m, dtype=bool)
    mask_r[[1, 7, 8, 20]] = True
    mask_c = torch.zeros(n, dtype=torch.bool)
    mask_c[[0, 5, 36]] = True
    ic.same_arrays(ic.expected(S, ("list", [1, 7, 8, 20]), ("list", [0, 5, 36])), _parts(A[mask_r][:, mask_c]))
    ic.same_arrays(ic.expected(S, ("list", [1, 7, 8, 20]), ("range", 2, 3, 4)), _parts(A[mask_r, 2:12:3]))
    R = S[mask_r][:, [0, 5, 36]]
    ic.same_arrays((R.indptr, R.indices, R.data), _parts(A[mask_r][:, mask_c]))


def test_empty_selections_ints_and_copies():
    S = ic.small()
    A = csr_matrix(S, device="cpu")
    m, n = S.shape
    for C, shape in ((A[5:5], (0, n)), (A[:, 9:3], (m, 0)), (A[[]], (0, n)), (A[:, []], (m, 0)),
                     (A[np.zeros(m, dtype=bool)], (0, n)), (A[4:4, 7:7], (0, 0))):
        assert C.shape == shape and C.nnz == 0 and C.indptr.tolist() == [0] * (shape[0] + 1)
    ic.same_arrays(ic.expected(S, ("range", 7, 1, 1), None), _parts(A[7]))
    assert A[7].shape == (1, n) and A[:, 3].shape == (m, 1) and A[-1].shape == (1, n)
    ic.same_arrays(ic.expected(S, None, ("range", n - 2, 1, 1)), _parts(A[:, -2]))
    ic.same_arrays(ic.expected(S, ("range", 7, 1, 1), ("list", [3, 3, 0])), _parts(A[7, [3, 3, 0]]))
    for C in (A[:], A[:, :], A[...], A[::1, 0:n]):
        assert C is not A and C.data.data_ptr() != A.data.data_ptr() and C._canonical is True
        ic.same_arrays((S.indptr, S.indices, S.data), _parts(C))


@pytest.mark.parametrize("dt", ic.DTYPES, ids=_name)
def test_element(dt):
    """A[i, j]: the sum of the stored duplicates as a Python scalar (scipy's _get_intXint)."""
    S = ic.small(dt)
    A = csr_matrix(S, device="cpu")
    D = S.toarray()
    for i, j in ((7, 0), (7, 36), (-16, -1), (4, 3), (0, 0), (22, 36)):
        v = A[i, j]
        assert isinstance(v, complex if np.dtype(dt).kind == "c" else float) and v == D[i, j]
    N = ic.noncanonical(np.float64)
    got = csr_matrix(N, device="cpu")[3, 5]
    e = [k for k in range(N.indptr[3], N.indptr[4]) if N.indices[k] == 5]
    assert len(e) == 3 and got == float(N.data[e].sum())
    assert csc_matrix(S.tocsc(), device="cpu")[7, 36] == D[7, 36]


def test_errors():
    A = csr_matrix(ic.small(), device="cpu")
    m, n = A.shape
    for key in ((m, 0), (0, n), (-m - 1, 0), ([0, m], slice(None)), (slice(None), [-n - 1]),
                (np.array([0.0, 1.0]), slice(None)), (slice(None), torch.tensor([1.5])),
                (np.zeros(m + 1, dtype=bool), slice(None)), (0, 0, 0), ([0, 1], [0, 1, 2]),
                (np.zeros((2, 2), dtype=np.int64), slice(None))):
        with pytest.raises(IndexError):
            A[key]
    with pytest.raises(NotImplementedError, match="pointwise"):
        A[[0, 1], [2, 3]]
    with pytest.raises(NotImplementedError, match="pointwise"):
        A[np.array([0, 1]), torch.tensor([2, 3])]
    with pytest.raises(NotImplementedError, match="pointwise"):
        csc_matrix(ic.small().tocsc(), device="cpu")[[0], [0]]


def test_canonical_flags():
    """True travels where the minor axis keeps its order; False never travels (a selection may
    leave out what made the source non-canonical: tests/test_canonical_flag_cpu.py): unknown."""
    for S, flag in ((ic.small(), True), (ic.noncanonical(), False)):
        A = csr_matrix(S, device="cpu")
        assert A._canonical is flag
        kept = True if flag else None
        assert A[3:9]._canonical is kept and A[[5, 0, 5]]._canonical is kept and A[::-2]._canonical is kept
        assert A[:, 3:20]._canonical is kept and A[:, 1::4]._canonical is kept and A[2, 5:6]._canonical is kept
        assert A[:, [4, 2]]._canonical is None and A[:, np.arange(5)]._canonical is None
        assert A[:, ::-1]._canonical is None and A[3:5, 20:2:-3]._canonical is None
        for sub, want in ((A[3:9], S[3:9]), (A[[5, 0, 5]], S[[5, 0, 5]]), (A[:, 1::4], S[:, 1::4]), (A[2, 5:6], S[2, 5:6])):
            fresh = sp.csr_matrix((want.data.copy(), want.indices.copy(), want.indptr.copy()), shape=want.shape)
            assert sub.has_canonical_format is bool(fresh.has_canonical_format)
    T = csc_matrix(ic.small().tocsc(), device="cpu")
    assert T._canonical is True
    assert T[:, [3, 1]]._canonical is True and T[2:9]._canonical is True      # the major axis of a CSC matrix
    assert T[[3, 1]]._canonical is None and T[::-1]._canonical in (None, False)


# ------------------------------------------------------------------ 3. special values
@pytest.mark.parametrize("dname", list(sv.DTYPES))
def test_special_values_keep_their_bits(dname):
    """-0.0, denormals, +-inf and NaNs with their sign and payload arrive bit for bit."""
    dt = sv.DTYPES[dname]
    S0 = ic.small(dt)
    rng = np.random.default_rng(7)
    data = sv.draw("mixed", (S0.nnz,), rng, dt, p_inf=0.05, p_nan=0.05)
    tiny = sv.draw("tiny", (S0.nnz,), rng, dt, scale=2.0 ** -12)
    data[::3] = tiny[::3]
    comp = data.view(sv.real_dtype(dt))
    u = ic.bits(comp)
    payload = (0x7FC12345, 0xFFC00001, 0x7F800001, 0xFFA5A5A5) if u.dtype == np.uint32 else \
        (0x7FF8000012345678, 0xFFF8000000000001, 0x7FF0000000000001, 0xFFF5A5A5A5A5A5A5)
    for k, pat in enumerate(payload):
        u[5 + 7 * k] = pat
    comp[1], comp[2] = -0.0, np.finfo(comp.dtype).smallest_subnormal
    assert np.isnan(comp).sum() >= 4 and np.isinf(comp).any() and (np.signbit(comp) & (comp == 0)).any()
    assert ((comp != 0) & (np.abs(comp) < np.finfo(comp.dtype).tiny)).any()
    S = sp.csr_matrix((data, S0.indices, S0.indptr), shape=S0.shape)
    A = csr_matrix(S, device="cpu")
    m, n = S.shape
    for rs, cs in ((("list", [7, 0, 7, 22]), None), (None, ("range", n - 1, -1, n)),
                   (("range", m - 1, -2, m // 2), ("list", [int(v) for v in rng.integers(0, n, 50)]))):
        C = A[ic.py_key(rs, m)][:, ic.py_key(cs, n)]
        ic.same_arrays(ic.expected(S, rs, cs), _parts(C))
