"""Inputs and the reference of the canonicalisation tests (spg_canonicalize_nnz /
spg_canonicalize, include/spgemm.h), shared by tests/test_canon_cpu.py and
tests/test_gpu_canonicalize.py.  A plain helper module (no pytest hooks); everything is generated
from seeds.

The reference is `restate`, the rule in numpy:
  SORT / SUM      np.lexsort((cols, rows)), which is stable: entries by (row, column), equal cells
                  in stored order; COO input with neither is grouped by a stable sort of the rows;
  SUM             per run of equal cells the first value copied, the later ones added one by one,
                  left to right, one numpy add (one rounding) each;
  DROP_ZEROS      `!= 0` on the result, applied last.
tests/test_canon_cpu.py pins it to scipy wherever scipy is determinate: the structure of SUM always,
DROP_ZEROS alone array for array, SORT without duplicates against sort_indices(), and the values of
SUM on inputs whose rows hold at most 16 stored entries or whose cells have multiplicity at most 2
(scipy's csr_sum_duplicates sorts each row with an unstable std::sort first, so beyond those its
order of addition is unspecified).
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp

from tests import special_values as sv

DTYPES = sv.DTYPES
SORT, SUM, DROP = 1, 2, 4


def rows_of(indptr):
    """The row of every stored entry of a CSR row pointer."""
    indptr = np.asarray(indptr, dtype=np.int64)
    return np.repeat(np.arange(indptr.size - 1, dtype=np.int64), np.diff(indptr))


def restate(shape, rows, cols, vals, ops, coo=False):
    """(indptr int64, indices int32, data) of the triplets after `ops` -- the rule above."""
    m = int(shape[0])
    rows, cols, vals = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64), np.asarray(vals)
    nnz = vals.size
    if ops & (SORT | SUM):
        order = np.lexsort((cols, rows))
    elif coo:
        order = np.argsort(rows, kind="stable")
    else:
        order = np.arange(nnz)
    r, c, v = rows[order], cols[order], vals[order]
    if ops & SUM and nnz:
        head = np.ones(nnz, dtype=bool)
        head[1:] = (r[1:] != r[:-1]) | (c[1:] != c[:-1])
        starts = np.flatnonzero(head)
        lens = np.diff(np.append(starts, nnz))
        out = v[starts].copy()           # the first value, its bits
        with np.errstate(all="ignore"):
            for k in range(1, int(lens.max())):
                sel = lens > k
                out[sel] = out[sel] + v[starts[sel] + k]
        r, c, v = r[starts], c[starts], out
    if ops & DROP:
        keep = v != 0
        r, c, v = r[keep], c[keep], v[keep]
    indptr = np.zeros(m + 1, dtype=np.int64)
    np.cumsum(np.bincount(r, minlength=m), out=indptr[1:])
    return indptr, c.astype(np.int32), v


def as_csr(m, rows, cols, vals):
    """The triplets as CSR arrays with every row in stored order (scipy's coo_tocsr): rows
    unsorted, duplicates kept.  Returns (indptr int64, indices int32, data)."""
    return restate((m, 0), rows, cols, vals, 0, coo=True)


def scipy_csr(shape, indptr, indices, data):
    """A scipy csr_matrix over copies of the arrays, no check and no sort."""
    M = sp.csr_matrix(shape, dtype=np.asarray(data).dtype)
    M.indptr, M.indices, M.data = (np.asarray(indptr).astype(np.int32), np.asarray(indices).astype(np.int32),
                                   np.array(data, copy=True))
    return M


def draw_values(rng, n, dt, decades=6.0):
    """n values of dtype dt spread over 2 * decades decades, so the order of a sum shows."""
    rd = sv.real_dtype(dt)

    def part():
        return (rng.standard_normal(n) * 10.0 ** rng.uniform(-decades, decades, n)).astype(rd)
    if np.dtype(dt).kind != "c":
        return part()
    out = np.empty(n, dtype=dt)
    out.real, out.imag = part(), part()
    return out


def pool_triplets(m, n, nnz, pool, dt, seed):
    """nnz triplets in shuffled order whose cells are drawn from `pool` random cells: any
    multiplicity, rows unsorted."""
    rng = np.random.default_rng(seed)
    pr, pc = rng.integers(0, m, pool), rng.integers(0, n, pool)
    pick = rng.integers(0, pool, nnz)
    return pr[pick], pc[pick], draw_values(rng, nnz, dt)


def mult2_triplets(m, n, cells, dup_share, dt, seed):
    """`cells` distinct cells, a share of them stored twice, in shuffled order: multiplicity <= 2."""
    rng = np.random.default_rng(seed)
    keys = np.unique(rng.integers(0, m * n, cells))
    twice = keys[rng.random(keys.size) < dup_share]
    keys = rng.permutation(np.concatenate([keys, twice]))
    return keys // n, keys % n, draw_values(rng, keys.size, dt)


def short_row_triplets(m, n, dt, seed):
    """Rows of 0..16 stored entries over at most 5 distinct columns each: multiplicities up to
    16, every row short enough for scipy's sort to be an insertion sort (stable)."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 17, m)
    rows = np.repeat(np.arange(m), lens)
    base = rng.integers(0, max(n - 5, 1), m)
    cols = np.minimum(base[rows] + rng.integers(0, 5, rows.size), n - 1)
    return rows, cols, draw_values(rng, rows.size, dt)


def order_pair(dt, seed=7):
    """Two COO inputs (shape, rows, cols, vals) with the same multiset of triplets in different
    stored orders whose sums differ: cell (3, 5) holds big, 1, -big, 1 in the first (big + 1 is
    big, so the sum is 1) and big, -big, 1, 1 in the second (2), among 500 other triplets."""
    m, n = 9, 11
    rows, cols, vals = pool_triplets(m, n, 500, 60, dt, seed)
    keep = ~((rows == 3) & (cols == 5))
    rows, cols, vals = rows[keep], cols[keep], vals[keep]
    big = 1e8 if sv.real_dtype(dt) == np.float32 else 1e17
    first = np.array([big, 1.0, -big, 1.0]).astype(dt)
    second = np.array([big, -big, 1.0, 1.0]).astype(dt)
    at = [10, 100, 200, 300]                 # scattered through the stored order
    out = []
    for four in (first, second):
        r, c, v = (np.insert(a, at, x) for a, x in ((rows, 3), (cols, 5), (vals, four)))
        out.append(((m, n), r, c, v))
    got = [restate(s, r, c, v, SUM, coo=True)[2] for s, r, c, v in out]
    assert not np.array_equal(got[0], got[1])
    return out


def distinct_triplets(m, n, cells, dt, seed):
    """Distinct cells in shuffled order (unsorted rows, no duplicates)."""
    return mult2_triplets(m, n, cells, 0.0, dt, seed)
