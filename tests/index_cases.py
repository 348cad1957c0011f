"""Submatrix extraction C = A[R, K] (spg_csr_extract_nnz / spg_csr_extract, include/spgemm.h; the
containers' __getitem__): the rule restated in numpy, the matrices and the case lists shared by
tests/test_index_cpu.py (the torch form and the containers, against scipy) and
tests/test_gpu_index.py (the kernels).  A plain helper module (no pytest hooks); everything is
generated from seeds and cached read-only.

A selection is ``None`` (the whole axis), ``("range", start, step, count)`` or ``("list", [...])``
with in-range, non-negative members.  The rule: output row i is source row sel_r(i) walked in
stored order; a stored entry (j, v) gives one entry (j, v) for K = None, one entry
((j - start) / step, v) when the range holds j, and for a list one entry (t, v) per position t
with idx[t] == j, positions ascending.
"""
from __future__ import annotations

import functools

import numpy as np
import scipy.sparse as sp

from tests.instantiations import seed_of

DTYPES = [np.float32, np.float64, np.complex64, np.complex128]


# ------------------------------------------------------------------ selections
def members(sel, extent):
    """The selected source indices, in order, as an int64 array."""
    if sel is None:
        return np.arange(extent, dtype=np.int64)
    if sel[0] == "range":
        _, start, step, count = sel
        return start + step * np.arange(count, dtype=np.int64)
    return np.asarray(sel[1], dtype=np.int64).reshape(-1)


def count_of(sel, extent):
    return int(members(sel, extent).size)


def py_key(sel, extent):
    """The selection as an indexing key for scipy and the containers: a slice or an int64 array."""
    if sel is None:
        return slice(None)
    if sel[0] == "range":
        _, start, step, count = sel
        if count == 0:
            return slice(0, 0)
        stop = start + step * count
        return slice(start, stop if stop >= 0 else None, step)
    return np.asarray(sel[1], dtype=np.int64).reshape(-1)


def has_repeat(sel):
    return sel is not None and sel[0] == "list" and len(set(sel[1])) != len(sel[1])


# ------------------------------------------------------------------ the rule
def restate(indptr, indices, data, rows, colsel, ncols):
    """(indptr int64, indices int32, data) of A[rows, colsel] by the rule of the module docstring.
    rows: the selected source rows in order (an int array); colsel: a selection over ncols columns."""
    where = {}
    if colsel is not None and colsel[0] == "list":
        for t, c in enumerate(colsel[1]):
            assert 0 <= int(c) < ncols
            where.setdefault(int(c), []).append(t)
    out_p, out_j, src = [0], [], []
    for r in np.asarray(rows, dtype=np.int64):
        for e in range(int(indptr[r]), int(indptr[r + 1])):
            j = int(indices[e])
            if colsel is None:
                outs = (j,)
            elif colsel[0] == "range":
                _, start, step, count = colsel
                d = j - start
                outs = (d // step,) if d % step == 0 and 0 <= d // step < count else ()
            else:
                outs = where.get(j, ())
            out_j.extend(outs)
            src.extend([e] * len(outs))
        out_p.append(len(out_j))
    return (np.asarray(out_p, dtype=np.int64), np.asarray(out_j, dtype=np.int32),
            np.asarray(data)[np.asarray(src, dtype=np.int64)])


def expected(S, rows_sel, cols_sel):
    """restate() of the scipy CSR matrix S for two selections."""
    return restate(S.indptr, S.indices, S.data, members(rows_sel, S.shape[0]), cols_sel, S.shape[1])


def bits(x):
    """The values as unsigned integers of their real component's width."""
    x = np.ascontiguousarray(x)
    return x.view(np.uint32 if x.dtype in (np.float32, np.complex64) else np.uint64)


def same_arrays(S, got, what=""):
    """got = (indptr, indices, data) equals S = (indptr, indices, data): the row pointer and the
    indices as numbers, the data on its integer bits and in its dtype."""
    sp_, sj, sx = S
    gp, gj, gx = (np.asarray(a) for a in got)
    assert np.array_equal(np.asarray(sp_, dtype=np.int64), gp.astype(np.int64)), f"{what}: row pointer"
    assert gj.dtype == np.int32 and np.array_equal(sj, gj), f"{what}: indices"
    assert gx.dtype == np.asarray(sx).dtype, f"{what}: dtype {gx.dtype}, expected {np.asarray(sx).dtype}"
    assert np.array_equal(bits(sx), bits(gx)), f"{what}: value bits"


# ------------------------------------------------------------------ matrices
def _frozen(S):
    for a in (S.data, S.indices, S.indptr):
        a.setflags(write=False)
    return S


def _values(rng, n, dt):
    v = rng.standard_normal(n)
    if np.dtype(dt).kind == "c":
        v = v + 1j * rng.standard_normal(n)
    return v.astype(dt)


@functools.lru_cache(maxsize=None)
def small(dt=np.float64):
    """23 x 37, canonical, rows 4 and 11 empty, row 7 full."""
    rng = np.random.default_rng(seed_of("index_cases", "small"))
    D = rng.random((23, 37)) < 0.2
    D[[4, 11]] = False
    D[7] = True
    S = sp.csr_matrix(D.astype(np.float64))
    S = sp.csr_matrix((_values(rng, S.nnz, dt), S.indices.astype(np.int32), S.indptr.astype(np.int32)), shape=S.shape)
    assert S.has_canonical_format
    return _frozen(S)


@functools.lru_cache(maxsize=None)
def noncanonical(dt=np.float64):
    """17 x 29 with unsorted rows and duplicate (row, column) entries; rows 0 and 9 empty."""
    rng = np.random.default_rng(seed_of("index_cases", "noncanonical"))
    lens = rng.integers(1, 12, 17)
    lens[[0, 9]] = 0
    cols = [rng.integers(0, 29, n) for n in lens]          # with replacement: duplicates, any order
    cols[3] = np.array([5, 5, 2, 5, 28, 2])
    indptr = np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.int32)
    indices = np.concatenate(cols).astype(np.int32)
    S = sp.csr_matrix((_values(rng, indices.size, dt), indices, indptr), shape=(17, 29))
    assert not S.has_canonical_format
    return _frozen(S)


MATRICES = {"small": small, "noncanonical": noncanonical}


def _selections(extent, rng):
    perm = rng.permutation(extent)
    e = extent
    return [
        None,
        ("range", 3, 1, 9),
        ("range", 0, 1, 0),
        ("range", e - 1, -1, e),                       # the whole axis reversed
        ("range", e - 2, -3, (e - 2) // 3 + 1),
        ("range", 2, 5, (e - 3) // 5 + 1),
        ("range", 6, 1, 1),
        ("list", []),
        ("list", [int(v) for v in perm]),
        ("list", [int(v) for v in perm[::-1][:7]]),
        ("list", [5, 0, 5, e - 1, 1, 5]),
        ("list", [2] * 9),
    ]


@functools.lru_cache(maxsize=None)
def cases():
    """[(id, matrix name, rows selection, cols selection)]: every pair of the row and the column
    selections above on both matrices."""
    out = []
    for name, make in MATRICES.items():
        m, n = make().shape
        rng = np.random.default_rng(seed_of("index_cases", "cases", name))
        for a, rs in enumerate(_selections(m, rng)):
            for b, cs in enumerate(_selections(n, rng)):
                out.append((f"{name}-r{a}-c{b}", name, rs, cs))
    return out


@functools.lru_cache(maxsize=None)
def random_cases(count=200):
    """Random selections (ranges with any step, lists with repeats) on both matrices."""
    rng = np.random.default_rng(seed_of("index_cases", "random"))

    def pick(extent):
        kind = rng.integers(0, 4)
        if kind == 0:
            return None
        if kind == 1:
            step = int(rng.choice([-4, -2, -1, 1, 2, 3]))
            start = int(rng.integers(0, extent))
            room = (start if step < 0 else extent - 1 - start) // abs(step) + 1
            return ("range", start, step, int(rng.integers(0, room + 1)))
        k = int(rng.integers(0, extent + 5))
        return ("list", [int(v) for v in (rng.integers(0, extent, k) if kind == 2 else rng.permutation(extent)[:k])])
    out = []
    for n in range(count):
        name = ("small", "noncanonical")[n % 2]
        m, k = MATRICES[name]().shape
        out.append((f"random{n}", name, pick(m), pick(k)))
    return out


# ------------------------------------------------------------------ the kernels' seams
SEAM_LENS = [0, 1, 63, 64, 65, 1023, 1024, 1025, 4097]
SEAM_SHAPE = (300, 5000)
SEAM_LONG = 8 * len(SEAM_LENS) - 1      # a row of 4097 entries


@functools.lru_cache(maxsize=None)
def seam_matrix(dt=np.float64):
    """300 x 5000, canonical: row 8 * n + 7 holds SEAM_LENS[n % 9] entries for n = 0 .. 35, every
    other row is empty -- lengths on each side of a wave (64), a wave's chunk (1024) and a
    workgroup (4096), empty rows between full ones; 29448 entries, 15 scan tiles of 2048."""
    rng = np.random.default_rng(seed_of("index_cases", "seam"))
    m, n = SEAM_SHAPE
    lens = np.zeros(m, dtype=np.int64)
    for k in range(36):
        lens[8 * k + 7] = SEAM_LENS[k % 9]
    cols = [np.sort(rng.choice(n, int(c), replace=False)) for c in lens]
    others = np.setdiff1d(np.arange(n), [17])              # the long row holds column 17, once
    cols[SEAM_LONG] = np.sort(np.append(rng.choice(others, 4096, replace=False), 17))
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    indices = np.concatenate(cols).astype(np.int32)
    S = sp.csr_matrix((_values(rng, indices.size, dt), indices, indptr), shape=(m, n))
    assert S.has_canonical_format and len(SEAM_LENS) == 9 and lens[SEAM_LONG] == 4097
    return _frozen(S)


@functools.lru_cache(maxsize=None)
def seam_cases():
    """[(id, rows selection, cols selection)] on seam_matrix()."""
    m, n = SEAM_SHAPE
    rng = np.random.default_rng(seed_of("index_cases", "seam-cases"))
    every = ("list", [int(v) for v in rng.permutation(n)])
    S = seam_matrix()
    short = [15, 23, 31, 39]                               # rows of 1, 63, 64 and 65 entries
    held = set(np.concatenate([S.indices[S.indptr[r]:S.indptr[r + 1]] for r in short]).tolist())
    absent = [c for c in range(n) if c not in held][:40]
    return [
        ("all_rows_all_cols", None, None),
        ("odd_span_all_cols", ("range", 16, 1, 200), None),           # the first source row starts at entry 1
        ("row_list_all_cols", ("list", [int(v) for v in rng.integers(0, m, 150)]), None),
        ("reversed_permutation", ("list", list(range(m - 1, -1, -1))), None),
        ("reversed_range_cols_range", ("range", m - 1, -1, m), ("range", 100, 1, 3000)),
        ("long_row_three_times", ("list", [SEAM_LONG, 3, SEAM_LONG, SEAM_LONG, 7]), None),
        ("long_row_three_times_stepped_cols", ("list", [SEAM_LONG, SEAM_LONG, 15, SEAM_LONG]), ("range", 1, 2, 2400)),
        ("cols_step_minus_3", None, ("range", n - 1, -3, (n - 1) // 3 + 1)),
        ("rows_step_2_cols_step_minus_3", ("range", 1, 2, 149), ("range", n - 2, -3, (n - 2) // 3 + 1)),
        ("column_130_times", ("list", [SEAM_LONG, 23, SEAM_LONG]), ("list", [17] * 130)),
        ("column_130_times_between_others", None, ("list", [int(v) for v in rng.permutation(600)[:70]] + [17] * 130 + [4000, 17])),
        ("every_column_permuted", ("range", 0, 3, 100), every),
        ("nothing_present", ("list", short + short[::-1]), ("list", absent)),
        ("one_row", ("range", SEAM_LONG, 1, 1), ("range", 0, 1, 2500)),
        ("mid_step_rows", ("list", [47, 39, 47, 23, 15, 55, 47]), ("range", 0, 7, 700)),
    ]


@functools.lru_cache(maxsize=None)
def duplicate_matrix(dt=np.float64):
    """40 x 64, non-canonical: every row holds its columns twice or three times, unsorted."""
    rng = np.random.default_rng(seed_of("index_cases", "duplicates"))
    cols = []
    for r in range(40):
        base = rng.choice(64, int(rng.integers(0, 30)), replace=False)
        c = np.concatenate([base, base, base[: len(base) // 2]])
        cols.append(rng.permutation(c))
    indptr = np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.int32)
    indices = np.concatenate(cols).astype(np.int32)
    S = sp.csr_matrix((_values(rng, indices.size, dt), indices, indptr), shape=(40, 64))
    return _frozen(S)
