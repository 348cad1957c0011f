"""The cached canonical flag (``csr_matrix._canonical`` / ``csc_matrix._canonical``: True, False or
None = unknown, resolved lazily) of every container a public operation returns or mutates, checked
against the truth recomputed from the result's own arrays.  The sources, the one list of operations
and the rule, shared by tests/test_canonical_flag_cpu.py (CPU tensors: the torch forms) and
tests/test_gpu_canonical_flag.py (device tensors: the engine).  A plain helper module (no pytest
hooks); everything is generated from fixed seeds.

The rule (``check``), for a result ``out`` and scipy's result of the same operation:

* the truth is tests/validate_cases.canon_status on out's arrays (a csc_matrix: read as the CSR of
  the transpose);
* ``out._canonical is True`` implies the truth is canonical, ``is False`` that it is not: the flag
  may be unknown, it may not lie;
* ``out.has_canonical_format == truth`` afterwards (a csc_matrix has no such attribute: through its
  free transpose), on CPU tensors as on device tensors;
* ``out.toarray()`` equals scipy's, compared with np.array_equal: all values are small integers
  (|v| <= 8) stored as floats, so every sum and product is exact and no order of addition shows;
* a copy of the result after ``sum_duplicates()`` is truly canonical and has the same ``toarray()``.

Sources (40 x 30, rows 0, 5, 6 and 38 empty): CAN canonical; UNS rows 2, 17 and 39 reversed; DUP
sorted with an adjacent duplicate in rows 9 and 26; MIX both, the pair of row 9 summing to an exact
zero and the pair of row 26 a stored zero beside its twin; ZTW canonical but for duplicates whose
twin is a stored zero (rows 9 and 26), so that ``eliminate_zeros()`` makes it canonical.  A csc
source is the same generator on 30 segments of 40, read as the CSC arrays of a 40 x 30 matrix.
"""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np
import scipy.sparse as sp
import torch

from spmm_amd.sparse import coo_matrix, csc_matrix, csr_matrix
from tests import validate_cases as vc

M, N, K = 40, 30, 35
KINDS = ("CAN", "UNS", "DUP", "MIX", "ZTW")
ENTRIES = ("scipy", "none", "flag")
B_KINDS = ("CAN", "MIX")
_REVERSED = {"UNS", "MIX"}
_DOUBLED = {"DUP", "MIX", "ZTW"}


# ------------------------------------------------------------------ sources
def _arrays(kind: str, n_major: int, n_minor: int, dt, seed: int):
    """(data, indices int32, indptr int32) of a source of this kind."""
    rng = np.random.default_rng(seed)
    empty = {0, 5, 6, n_major - 2}
    special = {2, 9, 17, 26, n_major - 1}
    cplx = np.dtype(dt).kind == "c"

    def value():
        v = int(rng.choice([-8, -5, -3, -2, -1, 1, 2, 3, 4, 7]))
        return complex(v, int(rng.integers(-8, 9))) if cplx else float(v)
    rows = []
    for i in range(n_major):
        n = 0 if i in empty else int(rng.integers(4, 7)) if i in special else int(rng.integers(0, 8))
        cols = sorted(int(c) for c in rng.choice(n_minor, n, replace=False))
        rows.append([(c, value()) for c in cols])
    if kind in _DOUBLED:
        for r in (9, 26):
            c, v = rows[r][1]
            if kind == "ZTW" or (kind == "MIX" and r == 26):
                twin = 0.0 * v                    # a stored zero beside its duplicate
            elif kind == "MIX":
                twin = -v                         # the pair sums to an exact zero
            else:
                twin = value()
            rows[r].insert(2 if r == 9 else 1, (c, twin))
    if kind in _REVERSED:
        for r in (2, 17, n_major - 1):
            rows[r].reverse()
    indptr = np.zeros(n_major + 1, dtype=np.int32)
    indptr[1:] = np.cumsum([len(r) for r in rows])
    indices = np.asarray([c for r in rows for c, _ in r], dtype=np.int32)
    data = np.asarray([v for r in rows for _, v in r], dtype=dt)
    return data, indices, indptr


@functools.lru_cache(maxsize=None)
def _frozen_arrays(kind, fmt, dt, shape=(M, N), salt=0):
    m, n = shape
    n_major, n_minor = (m, n) if fmt == "csr" else (n, m)
    seed = 7919 * KINDS.index(kind) + 101 * (fmt == "csc") + 13 * (np.dtype(dt).kind == "c") + salt + 1
    arrays = _arrays(kind, n_major, n_minor, dt, seed)
    for a in arrays:
        a.setflags(write=False)
    return arrays


def source(kind: str, fmt: str = "csr", dt=np.float64, shape=(M, N), salt=0):
    """A NEW scipy matrix of this kind each time (csr or csc; the arrays taken as they are)."""
    data, indices, indptr = (a.copy() for a in _frozen_arrays(kind, fmt, np.dtype(dt), shape, salt))
    return (sp.csr_matrix if fmt == "csr" else sp.csc_matrix)((data, indices, indptr), shape=shape)


def truth_of_arrays(indptr, indices, n_minor: int) -> bool:
    return vc.canon_status(np.asarray(indptr), np.asarray(indices), n_minor, len(indices)) == 1


def noncanonical_segments(S):
    """The rows (csr) or columns (csc) of a scipy matrix that are not strictly ascending."""
    p, j = S.indptr, S.indices
    return [i for i in range(len(p) - 1) if any(j[q] <= j[q - 1] for q in range(p[i] + 1, p[i + 1]))]


def enter(S, entry: str, dev):
    """The scipy csr / csc / coo matrix S as a container on ``dev``: from the scipy matrix, from its
    arrays with the flag unknown, or from its arrays with the truthful flag."""
    if S.format == "coo":
        return coo_matrix(S, device=dev)
    cls = csr_matrix if S.format == "csr" else csc_matrix
    if entry == "scipy":
        return cls(S, device=dev)
    n_minor = S.shape[1] if S.format == "csr" else S.shape[0]
    flag = None if entry == "none" else truth_of_arrays(S.indptr, S.indices, n_minor)
    return cls((S.data.copy(), S.indices.copy(), S.indptr.copy()), shape=S.shape, device=dev, canonical=flag)


# ------------------------------------------------------------------ the rule
def _host(t):
    return t.detach().cpu().numpy()


def truth_of(out) -> bool:
    n_minor = out.shape[1] if out.format == "csr" else out.shape[0]
    return truth_of_arrays(_host(out.indptr), _host(out.indices), n_minor)


def check(out, want):
    """The rule of the module docstring for one result.  ``want``: scipy's result, sparse or dense."""
    want = np.asarray(want.toarray() if sp.issparse(want) else want)
    if isinstance(out, torch.Tensor):            # a dense product: the values alone
        got = _host(out)
        assert got.shape == want.shape and np.array_equal(got, want), "values"
        return
    assert tuple(out.shape) == want.shape, f"shape {tuple(out.shape)}, scipy {want.shape}"
    if isinstance(out, coo_matrix):              # no flag of its own: the values, then its CSR form
        assert np.array_equal(out.toarray(), want), "values (coo)"
        out = out.tocsr()
    assert isinstance(out, (csr_matrix, csc_matrix))
    truth, flag = truth_of(out), out._canonical
    assert flag is True or flag is False or flag is None
    assert not (flag is True and not truth), "the flag says canonical, the arrays are not"
    assert not (flag is False and truth), "the flag says not canonical, the arrays are"
    c = out.copy() if out.format == "csr" else out.transpose(copy=True)   # (before the flag is resolved)
    resolved = out.has_canonical_format if out.format == "csr" else out.transpose().has_canonical_format
    assert resolved is truth, f"has_canonical_format {resolved!r}, the arrays say {truth}"
    assert np.array_equal(out.toarray(), want), "values"
    c.sum_duplicates()
    assert truth_of(c) and c._canonical is True, "not canonical after sum_duplicates()"
    assert np.array_equal(c.toarray(), want if out.format == "csr" else want.T), "values after sum_duplicates()"


def row_multisets(p, j, x):
    x = np.ascontiguousarray(x)
    b = x.view(np.uint32 if x.dtype in (np.float32, np.complex64) else np.uint64).reshape(len(j), -1)
    return [sorted((int(j[e]), tuple(int(w) for w in b[e])) for e in range(p[r], p[r + 1])) for r in range(len(p) - 1)]


def check_sorted(A, S):
    """A after A.sort_indices() against scipy's S after S.sort_indices(): the three arrays (rows
    with duplicates as multisets of (column, value bits): scipy's sort is not stable)."""
    p, j, x = _host(A.indptr), _host(A.indices), _host(A.data)
    assert len(j) == S.nnz, f"{len(j)} stored entries, scipy keeps {S.nnz}"
    assert np.array_equal(p.astype(np.int64), S.indptr.astype(np.int64)), "row pointer"
    assert x.dtype == S.data.dtype
    if len(noncanonical_segments(S)) == 0:
        assert np.array_equal(j, S.indices) and np.array_equal(x, S.data), "arrays"
    else:
        assert all(j[q] >= j[q - 1] for r in range(len(p) - 1) for q in range(p[r] + 1, p[r + 1])), "a row is not sorted"
        assert row_multisets(p, j, x) == row_multisets(S.indptr, S.indices, S.data), "rows as multisets"


# ------------------------------------------------------------------ operands
class Env:
    """What one call of an operation gets beside A: the second operand and the dense ones, built
    for one device, value type and kind of B.  Scipy operands are new objects on every access."""

    def __init__(self, dev, dt, b_kind="CAN"):
        self.dev, self.dt, self.b_kind = torch.device(dev), np.dtype(dt), b_kind
        rng = np.random.default_rng(5)
        self.D = rng.integers(-2, 3, (M, N)).astype(np.float64)       # dense operands, zeros among them
        self.Drow, self.Dcol = self.D[3:4].copy(), self.D[:, 4:5].copy()
        self.x = rng.integers(-3, 4, N).astype(dt)
        self.X = rng.integers(-3, 4, (N, 5)).astype(dt)

    def Bs(self):
        return source(self.b_kind, "csr", self.dt, (M, N), salt=1000)

    def B(self):
        return enter(self.Bs(), "none", self.dev)

    def Bms(self):
        return source(self.b_kind, "csr", self.dt, (N, K), salt=2000)

    def Bm(self):
        return enter(self.Bms(), "none", self.dev)

    def t(self, a):
        return torch.from_numpy(a.copy()).to(self.dev)


# ------------------------------------------------------------------ operations
# name; the formats of A it exists for; call(A, env) on a container; ref(S, env) on the scipy matrix;
# binary: run with B of both kinds; engine: needs the engine (on CPU tensors it must answer "is not
# available", after canonicalising its operands); sort: compared with check_sorted
Op = namedtuple("Op", "name call ref formats binary engine sort", defaults=(("csr",), False, False, False))
BOTH = ("csr", "csc")
ALL = ("csr", "csc", "coo")


def _cls(A):
    return csr_matrix if A.format == "csr" else csc_matrix


def _inplace(method):
    def call(A, env):
        getattr(A, method)()
        return A

    def ref(S, env):
        getattr(S, method)()
        return S
    return call, ref


def _index(name, key, formats=BOTH):
    return Op(name, lambda A, e: A[key(A) if callable(key) else key], lambda S, e: S[key(S) if callable(key) else key], formats)


def _good_major(S):
    """The key that keeps every canonical row (csr) or column (csc) and leaves the others out."""
    bad = set(noncanonical_segments(S))
    keep = [i for i in range(S.shape[0] if S.format == "csr" else S.shape[1]) if i not in bad]
    return keep if S.format == "csr" else (slice(None), keep)


def _good_key(A):
    if sp.issparse(A):
        return _good_major(A)
    S = (sp.csr_matrix if A.format == "csr" else sp.csc_matrix)(
        (_host(A.data), _host(A.indices), _host(A.indptr)), shape=A.shape)
    return _good_major(S)


_ROW_MASK = np.arange(M) % 3 != 1
_COL_MASK = np.arange(N) % 4 != 2
_COLS_ASC, _COLS_ANY, _COLS_REP = [1, 4, 9, 10, 22, 29], [22, 4, 29, 1, 10, 9], [4, 1, 4, 29, 4, 10, 1]

OPS = [
    # copies and casts
    Op("copy", lambda A, e: A.copy(), lambda S, e: S.copy(), BOTH),
    Op("constructor", lambda A, e: _cls(A)(A), lambda S, e: S.copy(), BOTH),
    Op("csr_matrix(other)", lambda A, e: csr_matrix(A), lambda S, e: S.tocsr(), ("csc", "coo")),
    Op("csc_matrix(other)", lambda A, e: csc_matrix(A), lambda S, e: S.tocsc(), ("csr", "coo")),
    Op("astype(complex128)", lambda A, e: A.astype(np.complex128), lambda S, e: S.astype(np.complex128)),
    Op("tocsr()", lambda A, e: A.tocsr(), lambda S, e: S.tocsr(), ALL),
    Op("tocsr(copy=True)", lambda A, e: A.tocsr(copy=True), lambda S, e: S.tocsr(copy=True)),
    Op("-A", lambda A, e: -A, lambda S, e: -S, ALL),
    Op("A*2", lambda A, e: A * 2, lambda S, e: S * 2, ALL),
    Op("2*A", lambda A, e: 2 * A, lambda S, e: 2 * S, BOTH),
    Op("multiply(2)", lambda A, e: A.multiply(2), lambda S, e: S.multiply(2), ALL),
    Op("multiply(D numpy)", lambda A, e: A.multiply(e.D), lambda S, e: S.multiply(e.D), BOTH),
    Op("multiply(D torch)", lambda A, e: A.multiply(e.t(e.D)), lambda S, e: S.multiply(e.D), BOTH),
    Op("multiply(row numpy)", lambda A, e: A.multiply(e.Drow), lambda S, e: S.multiply(e.Drow), BOTH),
    Op("multiply(row torch)", lambda A, e: A.multiply(e.t(e.Drow)), lambda S, e: S.multiply(e.Drow), BOTH),
    Op("multiply(column numpy)", lambda A, e: A.multiply(e.Dcol), lambda S, e: S.multiply(e.Dcol), BOTH),
    Op("multiply(column torch)", lambda A, e: A.multiply(e.t(e.Dcol)), lambda S, e: S.multiply(e.Dcol), BOTH),
    # binary operations
    Op("multiply(B)", lambda A, e: A.multiply(e.B()), lambda S, e: S.multiply(e.Bs()), ALL, True),
    Op("maximum(B)", lambda A, e: A.maximum(e.B()), lambda S, e: S.maximum(e.Bs()), BOTH, True),
    Op("minimum(B)", lambda A, e: A.minimum(e.B()), lambda S, e: S.minimum(e.Bs()), BOTH, True),
    Op("A+B", lambda A, e: A + e.B(), lambda S, e: S + e.Bs(), ALL, True),
    Op("A-B", lambda A, e: A - e.B(), lambda S, e: S - e.Bs(), BOTH, True),
    Op("A@B", lambda A, e: A @ e.Bm(), lambda S, e: S @ e.Bms(), ALL, True, True),
    Op("A@x", lambda A, e: A @ e.t(e.x), lambda S, e: S @ e.x, ALL, False, True),
    Op("A@X", lambda A, e: A @ e.t(e.X), lambda S, e: S @ e.X, ALL, False, True),
    # transposes and formats
    Op("T", lambda A, e: A.T, lambda S, e: S.T, BOTH),
    Op("transpose()", lambda A, e: A.transpose(), lambda S, e: S.transpose(), BOTH),
    Op("transpose(copy=True)", lambda A, e: A.transpose(copy=True), lambda S, e: S.transpose(copy=True), BOTH),
    Op("tocsc()", lambda A, e: A.tocsc(), lambda S, e: S.tocsc(), BOTH),
    Op("tocsc().tocsr()", lambda A, e: A.tocsc().tocsr(), lambda S, e: S.tocsc().tocsr(), BOTH),
    Op("tocsr().tocsc()", lambda A, e: A.tocsr().tocsc(), lambda S, e: S.tocsr().tocsc(), BOTH),
    Op("transpose_csr()", lambda A, e: A.transpose_csr(), lambda S, e: S.T.tocsr()),
    Op("tocsc().T", lambda A, e: A.tocsc().T, lambda S, e: S.tocsc().T, BOTH),
    Op("tocsr().T", lambda A, e: A.tocsr().T, lambda S, e: S.tocsr().T, BOTH),
    Op("T.tocsr()", lambda A, e: A.T.tocsr(), lambda S, e: S.T.tocsr(), BOTH),
    Op("T.tocsc()", lambda A, e: A.T.tocsc(), lambda S, e: S.T.tocsc(), BOTH),
    # in place
    Op("sum_duplicates()", *_inplace("sum_duplicates"), ("csr", "coo")),
    Op("eliminate_zeros()", *_inplace("eliminate_zeros"), ("csr", "coo")),
    Op("sort_indices()", *_inplace("sort_indices"), ("csr",), False, False, True),
    # the dense boundary
    Op("csr_matrix(D)", lambda A, e: _dense_ctor("csr", A, e), lambda S, e: sp.csr_matrix(S.toarray()), BOTH),
    Op("csc_matrix(D)", lambda A, e: _dense_ctor("csc", A, e), lambda S, e: sp.csc_matrix(S.toarray()), BOTH),
    Op("csr_matrix(A.todense())", lambda A, e: csr_matrix(A.todense()),
       lambda S, e: sp.csr_matrix(S.toarray()), ALL),
    # indexing
    _index("A[3]", 3),
    _index("A[:, 4]", (slice(None), 4)),
    _index("A[3:20]", slice(3, 20)),
    _index("A[::3]", slice(None, None, 3)),
    _index("A[::-1]", slice(None, None, -1)),
    _index("A[:, 2:17]", (slice(None), slice(2, 17))),
    _index("A[:, ::2]", (slice(None), slice(None, None, 2))),
    _index("A[:, ::-1]", (slice(None), slice(None, None, -1))),
    _index("A[:, ascending list]", (slice(None), _COLS_ASC)),
    _index("A[:, unsorted list]", (slice(None), _COLS_ANY)),
    _index("A[:, list with repeats]", (slice(None), _COLS_REP)),
    _index("A[row list]", [7, 2, 39, 7, 0]),
    _index("A[row mask]", _ROW_MASK),
    _index("A[:, column mask]", (slice(None), _COL_MASK)),
    _index("A[the canonical rows or columns]", _good_key),
    _index("A[3:20, 2:17]", (slice(3, 20), slice(2, 17))),
]
OP_IDS = [op.name for op in OPS]
assert len(set(OP_IDS)) == len(OP_IDS)


def _dense_ctor(fmt, A, env):
    S = (sp.csr_matrix if A.format == "csr" else sp.csc_matrix)(
        (_host(A.data), _host(A.indices), _host(A.indptr)), shape=A.shape)
    return (csr_matrix if fmt == "csr" else csc_matrix)(env.t(S.toarray()))


def scipy_source(kind, fmt, dt):
    """A new scipy source in this format (coo: the csr source's entries in stored order)."""
    return source(kind, "csr", dt).tocoo() if fmt == "coo" else source(kind, fmt, dt)


def run_one(op: Op, kind: str, fmt: str, entry: str, env: Env):
    """One operation on one source: the rule, or for an operation that needs the engine on CPU
    tensors the refusal it owes."""
    A = enter(scipy_source(kind, fmt, env.dt), entry, env.dev)
    S = scipy_source(kind, fmt, env.dt)
    if op.engine and env.dev.type != "cuda":
        try:
            op.call(A, env)
        except RuntimeError as err:              # the product runs only in the library
            assert "is not available" in str(err), f"{type(err).__name__}: {err}"
            return
        raise AssertionError("a product of CPU tensors did not refuse")
    out = op.call(A, env)
    want = op.ref(S, env)
    if op.sort:
        check_sorted(out, want)
    check(out, want)


def sweep(op: Op, dev, dt, entries=ENTRIES, kinds=KINDS):
    """Every source, entry and format of one operation: the list of what failed, as text."""
    failures = []
    for b_kind in (B_KINDS if op.binary else ("CAN",)):
        env = Env(dev, dt, b_kind)
        for fmt in op.formats:
            for kind in kinds:
                for entry in (entries if fmt != "coo" else entries[:1]):
                    label = f"{op.name} [{fmt} {kind} entered:{entry}" + (f" B:{b_kind}]" if op.binary else "]")
                    try:
                        run_one(op, kind, fmt, entry, env)
                    except (AssertionError, AttributeError, TypeError, NotImplementedError) as err:
                        failures.append(f"{label}: {type(err).__name__}: {err}")
                    except RuntimeError as err:
                        if "needs device-resident operands" not in str(err):
                            raise                # anything the device reports ends the sweep
                        failures.append(f"{label}: RuntimeError: {err}")
    return failures
