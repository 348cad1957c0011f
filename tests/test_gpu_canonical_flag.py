"""The cached canonical flag on device tensors, where the engine serves: the list of
tests/canonical_flag_cases.OPS under that module's rule (as tests/test_canonical_flag_cpu.py runs it
on CPU tensors), and the entry points of spmm_amd.cusparse that only exist for device tensors.

Bar: a flag may be unknown, it may not lie; ``has_canonical_format`` (spg_validate_csr) resolves it
to the truth recomputed from the result's own arrays; the values are scipy's, compared exactly
(small integers: every sum and product is exact).
"""
import itertools

import numpy as np
import pytest
import scipy.sparse as sp

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import canonical_flag_cases as fc          # noqa: E402

DEV = "cuda:0"


# ------------------------------------------------------------------ the list
@pytest.mark.parametrize("op", fc.OPS, ids=fc.OP_IDS)
def test_flag_never_lies_f64(op):
    failures = fc.sweep(op, DEV, np.float64)
    assert not failures, "\n" + "\n".join(failures)


@pytest.mark.parametrize("op", fc.OPS, ids=fc.OP_IDS)
def test_flag_never_lies_c64(op):
    """One pass over the list with complex64 values, every source entered with the flag unknown."""
    failures = fc.sweep(op, DEV, np.complex64, entries=("none",))
    assert not failures, "\n" + "\n".join(failures)


def test_the_engine_served():
    """The sweep above ran on the engine's entry points, not on the torch forms."""
    from spmm_amd import _lib
    from spmm_amd.sparse import _engine_has
    t = torch.zeros(1, device=DEV)
    for group in (_lib.CSR2CSC, _lib.CSRGEAM, _lib.CANONICALIZE, _lib.EXTRACT, _lib.DENSE_CONVERT, _lib.ELEMENTWISE,
                  ("spg_validate_csr",)):
        assert _engine_has(t, group, fc.M)


# ------------------------------------------------------------------ device-only entry points
def _sources(entries=fc.ENTRIES, fmt="csr", dt=np.float64):
    for kind, entry in itertools.product(fc.KINDS, entries):
        yield f"{fmt} {kind} entered:{entry}", kind, fc.enter(fc.scipy_source(kind, fmt, dt), entry, DEV), \
            fc.scipy_source(kind, fmt, dt)


@pytest.mark.parametrize("sort,sum_duplicates,eliminate_zeros", list(itertools.product((False, True), repeat=3)))
def test_canonicalize(sort, sum_duplicates, eliminate_zeros):
    """cusparse.canonicalize, csr and coo input, the eight combinations: scipy's sort_indices() /
    sum_duplicates() / eliminate_zeros() in that order (summing sorts; a COO input is grouped by
    row at least).  Without a sum the stored entries stay, the zeros apart."""
    from spmm_amd import cusparse
    for fmt in ("csr", "coo"):
        for label, kind, A, S in _sources(fc.ENTRIES if fmt == "csr" else ("scipy",), fmt):
            before = A.nnz
            out = cusparse.canonicalize(A, sort=sort, sum_duplicates=sum_duplicates, eliminate_zeros=eliminate_zeros)
            assert out is not A and out.format == "csr" and A.nnz == before, label
            want = S.toarray()
            fc.check(out, want)
            R = fc.scipy_source(kind, "csr", np.float64)          # the stored entries, by row
            if sum_duplicates:
                R.sum_duplicates()
            elif sort:
                R.sort_indices()
            if eliminate_zeros:
                R.eliminate_zeros()
            assert out.nnz == R.nnz, f"{label}: {out.nnz} stored entries, scipy {R.nnz}"
            assert np.array_equal(out.indptr.cpu().numpy(), R.indptr), label
            if sort or sum_duplicates:
                j, p = out.indices.cpu().numpy(), R.indptr
                assert all(j[q] >= j[q - 1] for r in range(fc.M) for q in range(p[r] + 1, p[r + 1])), label
            if sum_duplicates:
                assert out._canonical is True, label


def test_csrsort():
    from spmm_amd import cusparse
    for label, kind, A, S in _sources():
        assert cusparse.csrsort(A) is None, label
        S.sort_indices()
        fc.check_sorted(A, S)
        assert A._canonical is (True if kind == "CAN" and "none" not in label else None), label
        fc.check(A, S)


def test_csr2csc_and_csc2csr():
    from spmm_amd import cusparse
    for label, kind, A, S in _sources():
        out = cusparse.csr2csc(A)
        assert out.format == "csc", label
        fc.check(out, S)
        want = S.tocsc()
        assert np.array_equal(out.indices.cpu().numpy(), want.indices), label      # stable: scipy's own arrays
        assert np.array_equal(out.data.cpu().numpy(), want.data), label
    for label, kind, A, S in _sources(fmt="csc"):
        out = cusparse.csc2csr(A)
        assert out.format == "csr", label
        fc.check(out, S)
        want = S.tocsr()
        assert np.array_equal(out.indices.cpu().numpy(), want.indices), label
        assert np.array_equal(out.data.cpu().numpy(), want.data), label


def test_dense_conversions():
    from spmm_amd import cusparse
    for kind in fc.KINDS:
        D = fc.source(kind).toarray()                 # (the sums of MIX and ZTW leave zeros in it)
        t = torch.from_numpy(D).to(DEV)
        for out, fmt in ((cusparse.dense2csr(t), "csr"), (cusparse.dense2csc(t), "csc"),
                         (cusparse.denseToSparse(t), "csr"), (cusparse.denseToSparse(t, format="csc"), "csc"),
                         (cusparse.denseToSparse(t, format="coo"), "coo"),
                         (cusparse.dense2csr(t.t().contiguous().t()), "csr")):
            assert out.format == fmt and out.nnz == np.count_nonzero(D), kind
            if fmt != "coo":
                assert out._canonical is True, kind
            fc.check(out, D)


def _unknown(kind, shape=(fc.M, fc.N), salt=0):
    S = fc.source(kind, "csr", np.float64, shape, salt)
    return fc.enter(S, "none", DEV), fc.source(kind, "csr", np.float64, shape, salt)


def test_direct_calls_on_operands_whose_flag_is_unknown():
    """csrgeam2, csrbinop, multiply_by_dense and spgemm called directly: a canonical operand with
    the flag unknown passes the gate (one device check) and the result is scipy's; an operand that
    is not canonical is stopped by it."""
    from spmm_amd import cusparse
    env = fc.Env(DEV, np.float64)
    A, SA = _unknown("CAN")
    B, SB = _unknown("CAN", salt=1000)
    Bm, SBm = _unknown("CAN", (fc.N, fc.K), salt=2000)
    assert A._canonical is None and B._canonical is None and Bm._canonical is None
    fc.check(cusparse.csrgeam2(A, B, 2, -3), 2 * SA - 3 * SB)
    assert A._canonical is True and B._canonical is True
    for name, ref in (("multiply", SA.multiply(SB)), ("maximum", SA.maximum(SB)), ("minimum", SA.minimum(SB))):
        A, _ = _unknown("CAN")
        B, _ = _unknown("CAN", salt=1000)
        fc.check(cusparse.csrbinop(A, B, name), ref)
    for alg in (1, 2, 3):
        A, _ = _unknown("CAN")
        Bm, _ = _unknown("CAN", (fc.N, fc.K), salt=2000)
        C = cusparse.spgemm(A, Bm, alg=alg)
        assert C._canonical is True
        fc.check(C, SA @ SBm)
    for kind in fc.KINDS:                                # multiply_by_dense keeps the structure, and the flag
        A, S = _unknown(kind)
        out = cusparse.multiply_by_dense(A, env.t(env.D))
        assert out._canonical is None and A._canonical is None
        fc.check(out, S.multiply(env.D))
        A = fc.enter(S, "flag", DEV)
        out = cusparse.multiply_by_dense(A, env.t(env.Drow))
        assert out._canonical is (kind == "CAN")
        fc.check(out, S.multiply(env.Drow))
    for kind in ("UNS", "DUP", "MIX", "ZTW"):
        for call in (lambda a, b, bm: cusparse.csrgeam2(a, b), lambda a, b, bm: cusparse.csrgeam2(b, a),
                     lambda a, b, bm: cusparse.csrbinop(a, b, "multiply"), lambda a, b, bm: cusparse.spgemm(a, bm),
                     lambda a, b, bm: cusparse.spmv(a, env.t(env.x)), lambda a, b, bm: cusparse.spmm(a, env.t(env.X))):
            A, _ = _unknown(kind)
            B, _ = _unknown("CAN", salt=1000)
            Bm, _ = _unknown("CAN", (fc.N, fc.K), salt=2000)
            with pytest.raises(AssertionError):
                call(A, B, Bm)
            assert A._canonical is False


def test_a_canonical_part_of_a_non_canonical_matrix_passes_the_gate():
    """The rows of UNS, DUP and MIX that are canonical, and ZTW without its zeros: valid operands of
    a direct call, although they come from a matrix flagged False."""
    from spmm_amd import cusparse
    from spmm_amd.sparse import csr_matrix
    Bm, SBm = _unknown("CAN", (fc.N, fc.K), salt=2000)
    for kind in ("UNS", "DUP", "MIX"):
        S = fc.source(kind)
        A = csr_matrix(S, device=DEV)
        assert A._canonical is False
        good = [i for i in range(fc.M) if i not in fc.noncanonical_segments(S)]
        sub = A[good]
        assert sub._canonical is None
        fc.check(cusparse.spgemm(sub, Bm), S[good] @ SBm)
        assert sub._canonical is True
    S = fc.source("ZTW")
    Z = csr_matrix(S, device=DEV)
    Z.eliminate_zeros()
    assert Z._canonical is None
    fc.check(cusparse.spgemm(Z, Bm), S @ SBm)
    x = np.arange(1.0, fc.N + 1)
    y = cusparse.spmv(Z, torch.from_numpy(x).to(DEV))
    assert np.array_equal(y.cpu().numpy(), S @ x)
