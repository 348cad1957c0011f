"""Element-wise multiply / maximum / minimum without a GPU (tests/elementwise_cases.py).

1. the rule: the torch forms the containers use on CPU tensors (sparse._binop_torch,
   sparse._mul_dense_torch) and the helper's plain-numpy restatement equal scipy on the edge pair,
   on its special-value variant and on the probe vectors: indptr and indices array for array, values
   under special_values.assert_same_special; complex products also against special_values.cmul;
2. the inputs' category conditions, from scipy alone;
3. the Python surface on CPU tensors: multiply / maximum / minimum for csr, csc and coo operands,
   dtype promotion, canonicalisation first, every dense shape as numpy and as torch input, scalars,
   and every out-of-scope case with its message.
"""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from spmm_amd import sparse
from spmm_amd.sparse import coo_matrix, csc_matrix, csr_matrix
from tests import elementwise_cases as ec
from tests import geam_cases as gc
from tests import special_values as sv

DTYPES = ec.DTYPES


def _cpu(S, cls=csr_matrix):
    if cls is csr_matrix:
        return csr_matrix((S.data.copy(), S.indices, S.indptr), shape=S.shape, device="cpu",
                          canonical=bool(S.has_canonical_format))
    return cls(S.copy(), device="cpu")


def _parts(m):
    return m.indptr.numpy(), m.indices.numpy(), m.data.numpy()


def _as_csr_parts(m):
    """(indptr, indices, data) of a result of any format, as scipy converts it to CSR."""
    if m.format == "csr":
        return _parts(m)
    S = m.get().tocsr()
    S.sort_indices()
    return S.indptr, S.indices, S.data


# ------------------------------------------------------------------ 1. the rule
@pytest.mark.parametrize("op", ec.OPS)
@pytest.mark.parametrize("special", [False, True], ids=["finite", "special"])
@pytest.mark.parametrize("dt", DTYPES, ids=gc.case_id)
def test_rule_equals_scipy(dt, special, op):
    A, B = ec.pair("edge", dt, special)
    ref = ec.reference("edge", dt, special, op)
    ec.assert_equal(ec.rule(A, B, op), ref)
    C = sparse._binop_torch(_cpu(A), _cpu(B), op)
    assert C._canonical is True and C.shape == A.shape and C.indptr.dtype == torch.int32
    ec.assert_equal(_parts(C), ref)


@pytest.mark.parametrize("dt", [np.complex64, np.complex128], ids=gc.case_id)
def test_complex_products_follow_cmul(dt):
    """The helper's array product is special_values.cmul entry by entry, and scipy's multiply on the
    shared entries is that product."""
    A, B = ec.pair("edge", dt, True)
    x, y = A.data[:400], B.data[:400]
    got = ec.cmul_arrays(x, y)
    for i in range(x.size):
        sv.assert_values_special(got[i:i + 1], sv.cmul(complex(x[i]), y[i:i + 1]), f"entry {i}")
    ec.assert_equal(ec.rule(A, B, "multiply"), ec.reference("edge", dt, True, "multiply"))


@pytest.mark.parametrize("name,op", [(n, op) for n, (_, _, want) in ec.PROBES.items() for op in want])
def test_probes(name, op):
    A, B, _ = ec.PROBES[name]
    ec.check_probe(name, op, ec.scipy_binop(A, B, op))
    ec.check_probe(name, op, ec.rule(A, B, op))
    ec.check_probe(name, op, _parts(sparse._binop_torch(_cpu(A), _cpu(B), op)))
    ec.check_probe(name, op, _parts(getattr(_cpu(A), op)(_cpu(B))))


# ------------------------------------------------------------------ 2. the inputs
@pytest.mark.parametrize("op", ec.OPS)
@pytest.mark.parametrize("special", [False, True], ids=["finite", "special"])
@pytest.mark.parametrize("dt", DTYPES, ids=gc.case_id)
def test_category_conditions(dt, special, op):
    ec.check_categories("edge", dt, special, op)


def test_values_have_their_shares():
    for dt in DTYPES:
        A, B = ec.pair("edge", dt)
        for S in (A, B):
            re = S.data.real
            assert 0.15 < (re < 0).mean() < 0.35                       # about a quarter negative
            assert 0.03 < (S.data == 0).mean() < 0.07                  # about 5 % explicit zeros ...
            assert np.signbit(re[S.data == 0]).any() and not np.signbit(re[S.data == 0]).all()   # ... of both signs
    # fp32: products of two nonzero values that are denormal, and that underflow to 0
    A, B = ec.pair("edge", np.float32)
    a, b = A.toarray(), B.toarray()
    with np.errstate(all="ignore"):
        prod = a * b
    both = (a != 0) & (b != 0)
    assert (both & (prod == 0)).sum() >= 10
    assert (both & (prod != 0) & (np.abs(prod) < np.finfo(np.float32).tiny)).sum() >= 10


# ------------------------------------------------------------------ 3. the Python surface
@pytest.mark.parametrize("op", ec.OPS)
@pytest.mark.parametrize("fmt_a,fmt_b", [("csr", "csr"), ("csc", "csc"), ("csr", "csc"), ("csc", "csr"),
                                         ("coo", "csr"), ("csr", "coo"), ("coo", "coo")])
def test_sparse_operands(fmt_a, fmt_b, op):
    cls = {"csr": csr_matrix, "csc": csc_matrix, "coo": coo_matrix}
    A, B = ec.pair("edge", np.float64, True)
    C = getattr(_cpu(A, cls[fmt_a]), op)(_cpu(B, cls[fmt_b]))
    assert C.format == ("csc" if fmt_a == "csc" else "csr") and C.shape == A.shape and C._canonical is True
    ec.assert_equal(_as_csr_parts(C), ec.reference("edge", np.float64, True, op))


@pytest.mark.parametrize("op", ec.OPS)
@pytest.mark.parametrize("da,db", [(np.float32, np.float64), (np.float64, np.complex64), (np.complex64, np.float32)],
                         ids=lambda d: np.dtype(d).name)
def test_mixed_dtypes_are_promoted(da, db, op):
    A, B = ec.pair("edge", da)[0], ec.pair("edge", db)[1]
    want = ec.scipy_binop(A, B, op)
    C = getattr(_cpu(A), op)(_cpu(B))
    assert C.dtype == np.promote_types(da, db) == want[2].dtype
    ec.assert_equal(_parts(C), want)


@pytest.mark.parametrize("op", ec.OPS)
def test_noncanonical_operand_is_summed_first(op):
    # row 0: (0: 1 + 2, 2: 4, 2: -4) against (0: -5, 1: 6, 2: 0.5); row 1: unsorted
    N = sp.csr_matrix((np.array([1.0, 4.0, 2.0, -4.0, 7.0, -1.0]), np.array([0, 2, 0, 2, 3, 1]), np.array([0, 4, 6])),
                      shape=(2, 4))
    P = sp.csr_matrix((np.array([-5.0, 6.0, 0.5, 2.0]), np.array([0, 1, 2, 1]), np.array([0, 3, 4])), shape=(2, 4))
    assert not N.has_canonical_format
    Ns = N.copy()
    Ns.sum_duplicates()
    want = ec.scipy_binop(Ns, P, op)
    dN = csr_matrix((N.data, N.indices, N.indptr), shape=N.shape, device="cpu", canonical=False)
    ec.assert_equal(_parts(getattr(dN, op)(_cpu(P))), want)
    dN = csr_matrix((N.data, N.indices, N.indptr), shape=N.shape, device="cpu", canonical=False)
    ec.assert_equal(_parts(getattr(_cpu(P), op)(dN)), ec.scipy_binop(P, Ns, op))


DENSE_SHAPES = ["full", "vector", "row", "col", "one"]


def _dense(rng, which, shape, dt):
    m, n = shape
    return ec.dense_operand(rng, {"full": (m, n), "vector": (n,), "row": (1, n), "col": (m, 1), "one": (1, 1)}[which], dt)


@pytest.mark.parametrize("as_torch", [False, True], ids=["numpy", "torch"])
@pytest.mark.parametrize("which", DENSE_SHAPES)
@pytest.mark.parametrize("fmt", ["csr", "csc", "coo"])
@pytest.mark.parametrize("dt", DTYPES, ids=gc.case_id)
def test_multiply_by_dense(dt, fmt, which, as_torch):
    A, _ = ec.pair("edge", dt, True)
    D = _dense(np.random.default_rng(5), which, A.shape, dt)
    want = ec.mul_dense_reference(A, D)
    dA = _cpu(A, {"csr": csr_matrix, "csc": csc_matrix, "coo": coo_matrix}[fmt])
    C = dA.multiply(torch.from_numpy(D.copy()) if as_torch else D)
    assert C.format == ("csc" if fmt == "csc" else "csr") and C.shape == A.shape and C.nnz == A.nnz
    assert C._canonical is True
    if fmt == "csc":
        assert C.data.data_ptr() != dA.data.data_ptr() and C.indices.data_ptr() != dA.indices.data_ptr()
        assert torch.equal(C.indices, dA.indices) and torch.equal(C.indptr, dA.indptr)
        S = sp.csc_matrix((C.data.numpy(), C.indices.numpy(), C.indptr.numpy()), shape=C.shape).tocsr()
        got = (S.indptr, S.indices, S.data)
    else:
        got = _parts(C)
    sv.assert_same_special(got, (A.indptr, A.indices, want))


def test_multiply_by_dense_keeps_a_noncanonical_structure_and_promotes():
    N = sp.csr_matrix((np.array([1.0, 4.0, 2.0, -4.0], dtype=np.float32), np.array([0, 2, 0, 2]), np.array([0, 4, 4])),
                      shape=(2, 3))
    dN = csr_matrix((N.data, N.indices, N.indptr), shape=N.shape, device="cpu", canonical=False)
    D = np.array([[2.0, 3.0, 0.0], [1.0, 1.0, 1.0]])
    C = dN.multiply(D)
    assert C.dtype == np.float64 and C._canonical is False      # the flag is kept
    assert C.indices.tolist() == [0, 2, 0, 2] and C.indptr.tolist() == [0, 4, 4]
    assert C.data.tolist() == [2.0, 0.0, 4.0, -0.0] and np.signbit(C.data.numpy()[3])


@pytest.mark.parametrize("fmt", ["csr", "csc", "coo"])
@pytest.mark.parametrize("dt", DTYPES, ids=gc.case_id)
def test_scalars(dt, fmt):
    A, _ = ec.pair("edge", dt, True)
    cls = {"csr": csr_matrix, "csc": csc_matrix, "coo": coo_matrix}[fmt]
    dA = _cpu(A, cls)
    for s, got in [(2.5, dA * 2.5), (2.5, 2.5 * dA), (2.5, dA.multiply(2.5)), (np.float32(2.5), dA.multiply(np.float32(2.5))),
                   (2.5, dA.multiply(torch.tensor(2.5))), (2.5, dA.multiply(np.array(2.5))),
                   (-1.5 + 2j, dA * (-1.5 + 2j)), (-1.5 + 2j, (-1.5 + 2j) * dA)]:
        rdt = np.result_type(dt, s)
        assert got.dtype == rdt and got.format == ("csc" if fmt == "csc" else "csr")
        assert got._canonical is True
        p, j, x = _as_csr_parts(got)
        assert np.array_equal(p, A.indptr) and np.array_equal(j, A.indices)
        sv.assert_values_special(x, sv.cmul(s, A.data.astype(rdt)))
    one = dA * 1
    assert one.data.data_ptr() != dA.data.data_ptr()
    assert np.array_equal(one.data.numpy().view(np.uint8), dA.data.numpy().view(np.uint8))
    if np.dtype(dt).kind != "c":     # scipy's own scalar product, where numpy cannot fuse anything
        with np.errstate(all="ignore"):
            sv.assert_values_special(_as_csr_parts(dA * 2.5)[2], (A * 2.5).data)


def test_out_of_scope_and_type_errors():
    A, B = ec.pair("edge", np.float64)
    dA, dB = _cpu(A), _cpu(B)
    m, n = A.shape
    msg = "expected scalar, dense matrix/vector or csr matrix"
    for op in ec.OPS:
        with pytest.raises(TypeError, match=msg):
            getattr(dA, op)("abc")
        with pytest.raises(TypeError, match=msg):
            getattr(dA, op)([1, 2, 3])
        with pytest.raises(TypeError, match=msg):
            getattr(_cpu(A, csc_matrix), op)(None)
        with pytest.raises(NotImplementedError, match="different shapes .broadcasting. is not supported"):
            getattr(dA, op)(_cpu(sp.csr_matrix((1, n), dtype=np.float64)))
        with pytest.raises(NotImplementedError, match="different shapes .broadcasting. is not supported"):
            getattr(_cpu(A, csc_matrix), op)(_cpu(sp.csr_matrix((m, 1), dtype=np.float64)))
    for op in ("maximum", "minimum"):
        for other in (0, 1.5, np.zeros(A.shape), torch.zeros(n)):
            with pytest.raises(NotImplementedError, match=f"{op} with a scalar or a dense operand is not supported"):
                getattr(dA, op)(other)
    row = _cpu(sp.csr_matrix(np.ones((1, n))))
    with pytest.raises(NotImplementedError, match="dense operand larger than the sparse matrix"):
        row.multiply(np.ones((m, n)))
    with pytest.raises(NotImplementedError, match="dense operand larger than the sparse matrix"):
        _cpu(sp.csr_matrix(np.ones((m, 1)))).multiply(np.ones(n))
    with pytest.raises(ValueError, match="inconsistent shapes"):
        dA.multiply(np.ones((m, n + 1)))
    with pytest.raises(ValueError, match="inconsistent shapes"):
        dA.multiply(np.ones(n - 1))
    with pytest.raises(ValueError, match="could not interpret dimensions"):
        dA.multiply(np.ones((1, m, n)))
    assert dA.multiply(np.ones(n, dtype=np.int32)).dtype == np.float64     # an integer operand is promoted
    for thunk in (lambda: dA / 2.0, lambda: dA / dB, lambda: 2.0 / dA):
        with pytest.raises(NotImplementedError, match="division of a sparse matrix is not supported"):
            thunk()
    for thunk in (lambda: dA == dB, lambda: dA != dB, lambda: dA < dB, lambda: dA <= 1.0, lambda: dA > np.zeros(A.shape),
                  lambda: dA >= dB, lambda: 0 < dA):
        with pytest.raises(NotImplementedError, match="comparison of sparse matrices is not supported"):
            thunk()
    assert (dA == None) is False and (dA != "x") is True and isinstance(hash(dA), int)   # noqa: E711
    assert dA.__mul__("abc") is NotImplemented and _cpu(A, csc_matrix).__mul__(dB) is NotImplemented
    from spmm_amd import cusparse
    with pytest.raises(ValueError, match="op must be one of multiply, maximum, minimum"):
        sparse._binop_torch(dA, dB, "divide")
    assert set(cusparse._BINOPS) == set(ec.OPS) and cusparse._BINOPS == ec.OP_CODE


def test_coo_star_takes_scalars_only():
    """`*` on a coo_matrix scales by a scalar and offers nothing else (products are `@`)."""
    A, B = ec.pair("edge", np.float64)
    cA = _cpu(A, coo_matrix)
    assert cA.__mul__(_cpu(B)) is NotImplemented and cA.__rmul__(_cpu(B)) is NotImplemented
    assert cA.__mul__(np.ones(A.shape[1])) is NotImplemented and cA.__mul__(torch.ones(A.shape[1], 2)) is NotImplemented
    with pytest.raises(TypeError):
        cA * _cpu(B)
    got = cA * 2.0
    assert got.format == "csr"
    sv.assert_same_special(_parts(got), (A.indptr, A.indices, A.data * 2.0))
