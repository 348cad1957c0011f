"""Element-wise multiply / maximum / minimum: matrices, references and the comparison shared by
tests/test_elementwise_cpu.py and tests/test_gpu_elementwise.py.

A plain helper module (no pytest hooks).  Everything is generated from seeds.

The rule (include/spgemm.h, spg_csr_binop; scipy's csr_binop_csr_canonical): over the union of the
two patterns r = op(a, b), an operand without the entry contributing +0, and (column, r) is kept iff
r != 0.  What "equal" means: indptr and indices equal scipy's A.multiply(B) / A.maximum(B) /
A.minimum(B) array for array, the values under special_values.assert_same_special (+-0, denormals
and +-inf bit for bit, NaN exactly where scipy has one).

Structures: geam_cases.edge_pair and geam_cases.long_pair.  Values are redrawn here per
(structure, dtype, variant): about a quarter negative, about 5 % of each operand an explicit +0 or
-0, and a third of the magnitudes around 2^-75, so that fp32 products of two of them are denormal
or underflow to 0.  The `special` variant additionally plants +-inf, NaN and denormals on shared,
A-only and B-only positions.
"""
from __future__ import annotations

import functools

import numpy as np
import scipy.sparse as sp

from tests import geam_cases as gc
from tests import special_values as sv

DTYPES = gc.DTYPES
OPS = ("multiply", "maximum", "minimum")
OP_CODE = {"multiply": 0, "maximum": 1, "minimum": 2}     # spg_binop_t
CATEGORIES = ("shared_kept", "shared_dropped", "a_only_kept", "a_only_dropped", "b_only_kept", "b_only_dropped")
MIN_PER_CATEGORY = 10
PLANTED = 60      # planted special values per operand and position class


def _reals(rng, n, rd):
    """n finite values: a third with magnitude 2^U(-90, -60), the rest standard normal; a quarter
    negative."""
    mag = np.abs(rng.standard_normal(n)) + 0.01
    small = rng.random(n) < 1 / 3
    mag = np.where(small, np.exp2(rng.uniform(-90.0, -60.0, n)), mag)
    sgn = np.where(rng.random(n) < 0.25, -1.0, 1.0)
    return (sgn * mag).astype(rd)


def draw(rng, n, dt):
    """n values of dtype dt; about 5 % explicit zeros, half of them -0 (complex: both parts)."""
    rd = sv.real_dtype(dt)
    v = _reals(rng, n, rd)
    zero = np.where(rng.random(n) < 0.5, 0.0, -0.0).astype(rd)
    is_zero = rng.random(n) < 0.05
    if np.dtype(dt).kind == "c":
        out = np.empty(n, dtype=dt)
        im = _reals(rng, n, rd)
        im = np.where(rng.random(n) < 0.5, im, -im)        # the imaginary part's sign is free
        out.real, out.imag = np.where(is_zero, zero, v), np.where(is_zero, zero, im)
        return out
    return np.where(is_zero, zero, v).astype(dt)


def _keys(S):
    n = max(S.shape[1], 1)
    return np.repeat(np.arange(S.shape[0], dtype=np.int64), np.diff(S.indptr)) * n + S.indices


def _plant(data, at, rng, dt):
    """The special values, in turn, at the entries `at` (complex: in the real or the imaginary part)."""
    rd = sv.real_dtype(dt)
    den = np.finfo(rd).tiny / 8
    cycle = np.array([np.inf, -np.inf, np.nan, den, -den], dtype=rd)
    vals = cycle[np.arange(at.size) % cycle.size]
    if np.dtype(dt).kind == "c":
        part = rng.random(at.size) < 0.5
        data.real[at] = np.where(part, vals, data.real[at])
        data.imag[at] = np.where(part, data.imag[at], vals)
    else:
        data[at] = vals


@functools.lru_cache(maxsize=None)
def pair(which, dt, special=False):
    """(A, B) on the structure `which` ("edge" or "long") with this module's values."""
    SA, SB = {"edge": gc.edge_pair, "long": gc.long_pair}[which](dt)
    rng = np.random.default_rng(sv.seed_of("elementwise", which, np.dtype(dt).name, special))
    xa, xb = draw(rng, SA.nnz, dt), draw(rng, SB.nnz, dt)
    if special:
        ka, kb = _keys(SA), _keys(SB)
        in_b, in_a = np.isin(ka, kb), np.isin(kb, ka)
        _plant(xa, rng.choice(np.flatnonzero(in_b), PLANTED, replace=False), rng, dt)    # shared, A's side
        _plant(xb, rng.choice(np.flatnonzero(in_a), PLANTED, replace=False), rng, dt)    # shared, B's side
        _plant(xa, rng.choice(np.flatnonzero(~in_b), PLANTED, replace=False), rng, dt)   # A-only
        _plant(xb, rng.choice(np.flatnonzero(~in_a), PLANTED, replace=False), rng, dt)   # B-only
    A = sp.csr_matrix((xa, SA.indices, SA.indptr), shape=SA.shape)
    B = sp.csr_matrix((xb, SB.indices, SB.indptr), shape=SB.shape)
    assert A.has_canonical_format and B.has_canonical_format and A.dtype == B.dtype == dt
    A.data.setflags(write=False)
    B.data.setflags(write=False)
    return A, B


def scipy_binop(A, B, op):
    """scipy's result as (indptr, indices, data)."""
    with np.errstate(all="ignore"):
        R = getattr(A, op)(B).tocsr()
    assert R.has_canonical_format and R.dtype == np.promote_types(A.dtype, B.dtype)
    return R.indptr, R.indices, R.data


@functools.lru_cache(maxsize=None)
def reference(which, dt, special, op):
    """scipy's result of a pair, computed once and never written."""
    ref = scipy_binop(*pair(which, dt, special), op)
    for a in ref:
        a.setflags(write=False)
    return ref


def cmul_arrays(x, y):
    """x * y element by element by special_values.cmul's rule: (ac - bd) + (ad + bc)i on the real
    parts, every product and sum rounded on its own."""
    if x.dtype.kind != "c":
        with np.errstate(all="ignore"):
            return x * y
    out = np.empty_like(x)
    with np.errstate(all="ignore"):
        out.real = x.real * y.real - x.imag * y.imag
        out.imag = x.real * y.imag + x.imag * y.real
    return out


def _less(x, y):
    if x.dtype.kind != "c":
        with np.errstate(all="ignore"):
            return x < y
    with np.errstate(all="ignore"):
        return np.where(x.real == y.real, x.imag < y.imag, x.real < y.real)


def nonzero_bits(r):
    """r != 0 on the bits without their signs."""
    c = np.ascontiguousarray(r).view(sv.real_dtype(r.dtype))
    bits = c.view(np.uint32 if c.dtype == np.float32 else np.uint64)
    keep = (bits & (np.uint32(0x7FFFFFFF) if c.dtype == np.float32 else np.uint64(0x7FFFFFFFFFFFFFFF))) != 0
    return keep.reshape(r.shape[0], -1).any(axis=1)


def rule(A, B, op):
    """The rule restated in plain numpy: (indptr, indices, data)."""
    m, n = A.shape
    ka, kb = _keys(A), _keys(B)
    keys = np.union1d(ka, kb)
    a = np.zeros(keys.size, dtype=A.dtype)
    b = np.zeros(keys.size, dtype=A.dtype)
    a[np.searchsorted(keys, ka)] = A.data
    b[np.searchsorted(keys, kb)] = B.data
    if op == "multiply":
        r = cmul_arrays(a, b)
    elif op == "maximum":
        r = np.where(_less(a, b), b, a)
    else:
        r = np.where(_less(b, a), b, a)
    keep = nonzero_bits(r)
    keys, r = keys[keep], r[keep]
    rows = keys // max(n, 1)
    indptr = np.zeros(m + 1, dtype=np.int64)
    indptr[1:] = np.cumsum(np.bincount(rows, minlength=m))
    return indptr, (keys - rows * max(n, 1)).astype(np.int32), r


def categories(A, B, ref):
    """Entries per category, from the two patterns and scipy's result alone."""
    ka, kb = _keys(A), _keys(B)
    n = max(A.shape[1], 1)
    kr = np.repeat(np.arange(A.shape[0], dtype=np.int64), np.diff(ref[0])) * n + ref[1]
    shared, a_only, b_only = np.intersect1d(ka, kb), np.setdiff1d(ka, kb), np.setdiff1d(kb, ka)
    out = {}
    for name, ks in (("shared", shared), ("a_only", a_only), ("b_only", b_only)):
        kept = int(np.isin(ks, kr).sum())
        out[name + "_kept"], out[name + "_dropped"] = kept, ks.size - kept
    assert sum(out.values()) == np.union1d(ka, kb).size and kr.size == sum(v for k, v in out.items() if "kept" in k)
    return out


def check_categories(which, dt, special, op):
    """The category conditions: every category holds at least MIN_PER_CATEGORY entries; for
    multiply a one-sided entry is kept only through a planted inf or NaN, so those two categories
    are required in the special variant and must be empty in the finite one."""
    got = categories(*pair(which, dt, special), reference(which, dt, special, op))
    for name in CATEGORIES:
        if op == "multiply" and name in ("a_only_kept", "b_only_kept") and not special:
            assert got[name] == 0, (op, np.dtype(dt).name, special, got)
        else:
            assert got[name] >= MIN_PER_CATEGORY, (op, np.dtype(dt).name, special, got)
    return got


def assert_equal(got, ref):
    """got, ref: (indptr, indices, data)."""
    assert np.asarray(got[2]).dtype == np.asarray(ref[2]).dtype
    sv.assert_same_special(got, ref)


# ------------------------------------------------------------------ the probes (verified against scipy 1.15.3)

def _row(d, n, dt):
    cols = np.array(sorted(d), dtype=np.int32)
    return sp.csr_matrix((np.array([d[c] for c in cols], dtype=dt), cols, np.array([0, cols.size])), shape=(1, n))


def _dense_row(v, dt):
    """A 1 x n canonical CSR with every element of v stored (zeros included)."""
    v = np.asarray(v, dtype=dt)
    return sp.csr_matrix((v, np.arange(v.size, dtype=np.int32), np.array([0, v.size])), shape=(1, v.size))


nan, inf = np.nan, np.inf
# (A, B, {op: (kept columns, values or None)})
PROBES = {
    "pair1": (_dense_row([nan, 1, nan, -0., 0., -1, 2, -3], np.float64),
              _dense_row([1, nan, nan, 0., -0., -0., 2, -3], np.float64),
              {"maximum": ([0, 1, 2, 6, 7], [nan, 1, nan, 2, -3]),
               "minimum": ([0, 1, 2, 5, 6, 7], [nan, 1, nan, -1, 2, -3]),
               "multiply": ([0, 1, 2, 6, 7], None)}),
    "pair2": (_row({0: inf, 2: 2, 3: -0.}, 5, np.float64), _row({2: 5, 3: 0., 4: 7}, 5, np.float64),
              {"multiply": ([0, 2], [nan, 10])}),
    "pair3": (_dense_row([1 + 2j, 1 + 2j, 0 - 1j], np.complex128), _dense_row([1 + 3j, 0 + 5j, 0j], np.complex128),
              {"maximum": ([0, 1], [1 + 3j, 1 + 2j]), "minimum": ([0, 1, 2], [1 + 2j, 5j, 0 - 1j])}),   # (0 - 1j: the literal -1j is -0-1j)
    "pair4": (_dense_row([1e-30, 1e-20], np.float32), _dense_row([1e-10, 1e-30], np.float32),
              {"multiply": ([0], [np.float32(1e-30) * np.float32(1e-10)])}),
}


def check_probe(name, op, got):
    """got: (indptr, indices, data) for PROBES[name] under op."""
    A, _, want = PROBES[name]
    cols, vals = want[op]
    assert np.asarray(got[0]).tolist() == [0, len(cols)] and np.asarray(got[1]).tolist() == cols, (name, op, got)
    if vals is not None:
        sv.assert_values_special(np.asarray(got[2]), np.array(vals, dtype=A.dtype), f"{name} {op}")


# ------------------------------------------------------------------ sparse times dense

def dense_operand(rng, shape, dt):
    """A dense operand with this module's values (zeros and small magnitudes included)."""
    return draw(rng, int(np.prod(shape)), dt).reshape(shape)


def mul_dense_reference(A, D):
    """A.data[e] * D[i, j] per stored entry, D broadcast to A's shape: scipy's A.multiply(D), which
    keeps every stored entry in A's stored order (as COO), for real types; for complex types the
    same entries by cmul_arrays."""
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    d = np.broadcast_to(D, A.shape)[rows, A.indices]
    want = cmul_arrays(A.data, d.astype(A.dtype))
    if A.dtype.kind != "c":
        with np.errstate(all="ignore"):
            R = A.multiply(D).tocoo()
        if A.has_canonical_format:
            assert np.array_equal(R.row, rows) and np.array_equal(R.col, A.indices)
            sv.assert_values_special(R.data, want, "scipy's multiply against the rule")
    return want
