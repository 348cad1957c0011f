"""Dense <-> CSR conversion: a numpy restatement of the two rules and the case builders shared by
tests/test_dense_cpu.py and tests/test_gpu_dense.py.

A plain helper module (no pytest hooks).  Everything is generated from seeds.

The rules (include/spgemm.h, spg_csr2dense and spg_dense2csr):
  todense    element (i, j) = 0 + v1 + v2 + ... over row i's stored entries with column j, in stored
             order, every add rounded on its own (numpy's complex add is part by part);
  fromdense  an element is kept iff its bits without the sign bit(s) are nonzero -- value != 0
             decided on the integers -- kept values are copied, columns ascend inside a row.

The kernels' constants (spmm_amd/csrc/spgemm_dense.hpp), mirrored here as test_gpu_csr2csc.py
mirrors the transpose's: W the columns of csr2dense's LDS window, R the rows of its band, S the
columns of a dense2csr segment, T the tile edge of dense2csr's column-major read.  The shapes
below sit on the seams of those constants.
"""
from __future__ import annotations

import functools

import numpy as np
import scipy.sparse as sp

WAVE, W, R, S, T = 64, 512, 8, 1024, 64
DTYPES = {"f32": np.float32, "f64": np.float64, "c64": np.complex64, "c128": np.complex128}


def real_dtype(dt):
    return np.dtype(dt).type(0).real.dtype


def bits(v):
    return np.ascontiguousarray(v).view(np.uint8)


# ------------------------------------------------------------------ the two rules in numpy
def ref_todense(A):
    """A (scipy CSR, taken as stored) as a dense array by the sequential rule."""
    m, n = A.shape
    out = np.zeros(m * n, dtype=A.dtype)
    if A.nnz == 0:
        return out.reshape(m, n)
    rows = np.repeat(np.arange(m, dtype=np.int64), np.diff(A.indptr))
    key = rows * n + A.indices.astype(np.int64)
    order = np.argsort(key, kind="stable")
    ks, vs = key[order], A.data[order]
    first = np.ones(ks.size, dtype=bool)
    first[1:] = ks[1:] != ks[:-1]
    start = np.maximum.accumulate(np.where(first, np.arange(ks.size), 0))
    rank = np.arange(ks.size) - start          # position of an entry among its element's entries
    with np.errstate(all="ignore"):
        for r in range(int(rank.max()) + 1):   # round r adds every element's r-th entry
            sel = rank == r
            out[ks[sel]] = out[ks[sel]] + vs[sel]
    return out.reshape(m, n)


def keep_mask(D):
    """True where an element's bits without the sign bit(s) are nonzero."""
    D = np.asarray(D)
    rd = real_dtype(D.dtype)
    u = np.uint32 if rd == np.float32 else np.uint64
    comps = np.ascontiguousarray(D).view(rd).view(u).reshape(D.shape + (-1,))
    mask = u(0x7FFFFFFF) if rd == np.float32 else u(0x7FFFFFFFFFFFFFFF)
    return ((comps & mask) != 0).any(axis=-1)


def ref_fromdense(D):
    """(indptr, indices, data) of csr_matrix(D) by the keep rule; data copied byte for byte."""
    D = np.asarray(D)
    keep = keep_mask(D)
    r, c = np.nonzero(keep)                    # row-major: columns ascend inside a row
    indptr = np.zeros(D.shape[0] + 1, dtype=np.int64)
    indptr[1:] = np.cumsum(keep.sum(axis=1))
    item = D.dtype.itemsize
    data = bits(D).reshape(D.shape + (item,))[r, c].reshape(-1).view(D.dtype)
    return indptr, c.astype(np.int32), data


# ------------------------------------------------------------------ values
def values(rng, n, dt):
    v = rng.standard_normal(n)
    if np.dtype(dt).kind == "c":
        v = v + 1j * rng.standard_normal(n)
    return v.astype(dt)


def special_pool(rd):
    """Components of the real type rd as bit patterns: quiet and signalling NaNs with payloads and
    both signs, +-0, the smallest denormal (both signs), a larger denormal, +-inf, normals."""
    if rd == np.float32:
        return np.array([0x7FC00001, 0xFFC00123, 0x7F800001, 0xFF800ABC, 0x00000000, 0x80000000, 0x00000001,
                         0x80000001, 0x00400000, 0x7F800000, 0xFF800000, 0x3F800000, 0xC0490FDB], dtype=np.uint32)
    return np.array([0x7FF8000000000001, 0xFFF8000000000123, 0x7FF0000000000001, 0xFFF0000000000ABC,
                     0x0000000000000000, 0x8000000000000000, 0x0000000000000001, 0x8000000000000001,
                     0x0008000000000000, 0x7FF0000000000000, 0xFFF0000000000000, 0x3FF0000000000000,
                     0xC00921FB54442D18], dtype=np.uint64)


def special_values(rng, n, dt, zero_share=0.3):
    """n values of dt whose components come from special_pool (complex: both parts drawn on their
    own, so values with one zero part and with two occur), `zero_share` of the components +-0."""
    rd = real_dtype(dt)
    pool = special_pool(rd)
    ncomp = 2 if np.dtype(dt).kind == "c" else 1
    comps = pool[rng.integers(0, pool.size, size=n * ncomp)]
    zeros = pool[4:6]
    z = rng.random(n * ncomp) < zero_share
    comps = np.where(z, zeros[rng.integers(0, 2, size=n * ncomp)], comps)
    return comps.view(rd).view(dt) if ncomp == 2 else comps.view(dt)


# ------------------------------------------------------------------ csr2dense cases
def _csr(rows_cols, rows_vals, n, dt):
    lens = [len(c) for c in rows_cols]
    indptr = np.zeros(len(lens) + 1, dtype=np.int32)
    indptr[1:] = np.cumsum(lens)
    cols = np.concatenate([np.asarray(c, dtype=np.int32) for c in rows_cols]) if sum(lens) else np.zeros(0, np.int32)
    vals = np.concatenate([np.asarray(v, dtype=dt) for v in rows_vals]) if sum(lens) else np.zeros(0, dt)
    return sp.csr_matrix((vals, cols, indptr), shape=(len(lens), n))


@functools.lru_cache(maxsize=None)
def lengths_case(dname, m, n):
    """m x n canonical CSR whose rows cycle through the lengths 0, 1, 63, 64, 65 and full (clipped
    to n), columns spread over the whole width."""
    dt = DTYPES[dname]
    rng = np.random.default_rng(1000 * m + n)
    cols, vals = [], []
    for i in range(m):
        k = min([0, 1, 63, 64, 65, n][(i + (1 if m == 1 else 0) * 5) % 6], n)
        c = np.sort(rng.choice(n, size=k, replace=False))
        if k >= 2:
            c[0], c[-1] = 0, n - 1            # the first and the last column are hit
        cols.append(c)
        vals.append(values(rng, k, dt))
    return _csr(cols, vals, n, dt)


TRIPLE = (1e16, 1.0, -1e16)   # in stored order sums to 0.0; any other order gives 1.0 or 2.0


@functools.lru_cache(maxsize=None)
def duplicates_case(dname):
    """12 x (2W + 1), not canonical.  Rows 0-5: multiplicities 2-5 inside one batch of 64; a pair
    straddling entries 63 and 64; pairs in the last column of window 0 and the first of window 1;
    an unsorted row with duplicates; a row of 200 entries that all hit one element; an empty row.
    Rows 6-10: the TRIPLE in each of those positions (adjacent in one batch, entries 62-64,
    63-65, one per window seam column, spread over an unsorted row).  Row 11: the TRIPLE four
    times on one element."""
    dt = DTYPES[dname]
    n = 2 * W + 1
    rng = np.random.default_rng(42)
    cols, vals = [], []

    def add(c, v=None):
        cols.append(np.asarray(c))
        vals.append(values(rng, len(c), dt) if v is None else np.asarray(v, dtype=dt))
    add([5, 5, 9, 9, 9, 12, 12, 12, 12, 20, 20, 20, 20, 20, 33, 700, 1024])
    base = np.sort(rng.choice(np.arange(1, n - 1), size=63, replace=False))
    add(np.concatenate([base, [base[-1] + 1, base[-1] + 1, 0]]))          # entries 63 and 64 alike
    add([W - 1, W, W - 1, W, 2 * W - 1, 2 * W, 2 * W, 2 * W - 1])
    c = rng.integers(0, n, size=150)
    add(np.concatenate([c, c[:40]])[rng.permutation(190)])
    add(np.full(200, W + 3))
    add([])
    one = dt(1.0)
    t = [dt(x) for x in TRIPLE]
    add([7, 7, 7, 8], t + [one])
    fillc = np.arange(100, 162)                                             # 62 distinct entries first
    add(np.concatenate([fillc, [3, 3, 3]]), [one] * 62 + t)                 # entries 62, 63, 64
    add(np.concatenate([fillc, [99], [3, 3, 3]]), [one] * 63 + t)           # entries 63, 64, 65
    add([W - 1, W, W - 1, W, W - 1, W], [t[0], t[0], t[1], t[1], t[2], t[2]])
    spread = rng.permutation(np.arange(10, 10 + 197))
    cc = np.concatenate([spread[:50], [600], spread[50:120], [600], spread[120:], [600]])
    vv = np.concatenate([values(rng, 50, dt), [t[0]], values(rng, 70, dt), [t[1]], values(rng, 77, dt), [t[2]]])
    add(cc, vv)
    add([2] * 12, t * 4)
    return _csr(cols, vals, n, dt)


TRIPLE_CELLS = [(6, 7), (7, 3), (8, 3), (9, W - 1), (9, W), (10, 600), (11, 2)]   # all sum to 0.0


@functools.lru_cache(maxsize=None)
def special_case(dname):
    """(R + 1) x (W + 1), not canonical: special values as lone entries and as summands (a third
    of the entries stored two to four times, rows shuffled)."""
    dt = DTYPES[dname]
    m, n = R + 1, W + 1
    rng = np.random.default_rng(7)
    cols = []
    for _ in range(m):
        c = rng.choice(n, size=90, replace=False)
        d = np.repeat(c[:30], rng.integers(1, 4, size=30))
        cols.append(rng.permutation(np.concatenate([c, d])))
    vals = [special_values(rng, len(c), dt) for c in cols]
    return _csr(cols, vals, n, dt)


TODENSE_SHAPES = sorted({(R + 1, n) for n in (1, 63, 64, 65, W - 1, W, W + 1, 2 * W + 1)} |
                        {(m, W + 1) for m in (1, R - 1, R, R + 1, 3 * R + 1)})


# ------------------------------------------------------------------ dense2csr cases
@functools.lru_cache(maxsize=None)
def dense_case(dname, m, n, kind="random"):
    """An m x n dense array.  random: 30 % normals, the rest +0.0, with special values (-0.0, for
    complex 0-0j and values with one zero part, denormals, NaNs with payloads, +-inf) in the first
    and last column of every segment of S columns and sprinkled elsewhere; zeros: all +-0;
    full: no element zero."""
    dt = DTYPES[dname]
    rng = np.random.default_rng(100000 * m + n)
    if kind == "zeros":
        D = np.zeros((m, n), dtype=dt)
        D.reshape(-1)[::3] = dt(-0.0) if np.dtype(dt).kind != "c" else dt(complex(0.0, -0.0))
        return D
    D = values(rng, m * n, dt).reshape(m, n)
    if kind == "full":
        return D
    D[rng.random((m, n)) >= 0.3] = 0
    seam = sorted({c for c in (0, S - 1, S, 2 * S - 1, 2 * S, n - 1) if 0 <= c < n})
    for c in seam:
        D[:, c] = special_values(rng, m, dt)
    k = max(1, m * n // 50)
    D.reshape(-1)[rng.choice(m * n, size=k, replace=False)] = special_values(rng, k, dt)
    return D


FROMDENSE_SHAPES = sorted({(R + 1, n) for n in (1, 63, 64, 65, S - 1, S, S + 1, 2 * S + 1)} |
                          {(m, 65) for m in (1, R - 1, R, R + 1, 3 * R + 1, T - 1, T, T + 1, 2 * T + 3)})
