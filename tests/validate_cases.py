"""The canonical-format check (spg_validate_csr / k_validate, include/spgemm.h; the torch form
behind ``csr_matrix.has_canonical_format``): the rule restated as Python loops, and the one list of
cases shared by tests/test_validate_cpu.py (the reference itself, the torch form) and
tests/test_gpu_validate.py (the kernel and the host decode).  A plain helper module (no pytest
hooks); every case is built from fixed patterns, nothing is random.

The kernel runs one thread per row in blocks of BLOCK = 256 threads, so the row counts sit on
each side of one block and one thread into the third, and single faults are placed in the first
and the last row and on both sides of the block seam (rows 255 and 256).

What a case may hold (so that no launch reads outside an allocation): ``indptr`` always has
rows + 1 entries and ``indices`` exactly ``nnz`` entries, the descriptor's nnz.  Only the VALUES of
indptr are ever wrong; a row whose pointers are bad (start < 0, end < start or end > nnz) is left
before any index is read, and every other row reads [start, end) inside [0, nnz).  Column values
out of range are compared, never used as addresses.  ``reads_stay_inside`` states this and both
test files assert it for every case.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

INT32_MAX = 2 ** 31 - 1
BLOCK = 256
ROW_COUNTS = (1, 255, 256, 257, 513)
COLS = 200
LONG = 65                                   # longer than a wave; to a per-thread kernel just "long"
_PATTERN = (2, 0, LONG, 1, 0, 0, 2, 1)      # canonical rows of 0, 1, 2 and 65 entries, mixed
_EDGE_RUN = 3                               # empty rows at the start and at the end (rows >= 16)


# ------------------------------------------------------------------ the rule
def canon_status(indptr, indices, cols, nnz) -> int:
    """spg_validate_csr's verdict by its contract: -1 if any row has p0 < 0, p1 < p0 or p1 > nnz,
    or if any index read in a well-formed row is outside [0, cols); otherwise 0 if any
    well-formed row has j[q] <= j[q-1]; otherwise 1."""
    bad = unordered = False
    for i in range(len(indptr) - 1):
        p0, p1 = int(indptr[i]), int(indptr[i + 1])
        if p0 < 0 or p1 < p0 or p1 > nnz:
            bad = True
            continue
        for q in range(p0, p1):
            c = int(indices[q])
            if c < 0 or c >= cols:
                bad = True
            if q > p0 and c <= int(indices[q - 1]):
                unordered = True
    return -1 if bad else 0 if unordered else 1


def well_formed_rows(indptr, nnz):
    """The rows whose pointers pass the kernel's first test, as (row, p0, p1)."""
    out = []
    for i in range(len(indptr) - 1):
        p0, p1 = int(indptr[i]), int(indptr[i + 1])
        if not (p0 < 0 or p1 < p0 or p1 > nnz):
            out.append((i, p0, p1))
    return out


def reads_stay_inside(case) -> bool:
    """Every index a launch on this case reads lies inside the allocated ``nnz`` entries, and the
    arrays have the sizes the descriptor states."""
    if len(case.indptr) != case.rows + 1 or len(case.indices) != case.nnz:
        return False
    return all(0 <= p0 and p1 <= case.nnz for _, p0, p1 in well_formed_rows(case.indptr, case.nnz))


def violating_pairs(indptr, indices):
    """[(row, entry within the row)] of every pair j[e] <= j[e-1] inside a row (well-formed input)."""
    out = []
    for i in range(len(indptr) - 1):
        for q in range(int(indptr[i]) + 1, int(indptr[i + 1])):
            if int(indices[q]) <= int(indices[q - 1]):
                out.append((i, q - int(indptr[i])))
    return out


def out_of_range(indices, cols):
    """The positions of the indices outside [0, cols)."""
    return [q for q, c in enumerate(indices) if int(c) < 0 or int(c) >= cols]


# ------------------------------------------------------------------ the builder
@dataclass(frozen=True, eq=False)
class Case:
    id: str
    rows: int
    cols: int
    indptr: np.ndarray            # int64, rows + 1 entries (cast to the row-pointer type under test)
    indices: np.ndarray           # int32, nnz entries
    expect: int                   # 1, 0 or -1
    kind: str                     # what the case claims (checked in tests/test_validate_cpu.py)
    at: tuple = ()                # the claim's position: (row, entry) of the single fault
    repaired: np.ndarray | None = field(default=None)   # the indices with the fault repaired: verdict 1

    @property
    def nnz(self) -> int:
        return int(self.indices.size)


def row_lengths(rows: int, forced=None):
    """The base row lengths: _PATTERN repeated, a run of empty rows at each end once there is
    room, and ``forced`` {row: length} on top."""
    lens = [_PATTERN[i % len(_PATTERN)] for i in range(rows)]
    if rows >= 16:
        for i in range(_EDGE_RUN):
            lens[i] = lens[rows - 1 - i] = 0
    for r, n in (forced or {}).items():
        lens[r] = n
    return lens


def _columns(i: int, n: int):
    """Row i's n canonical columns: start 1 .. 7, step 2 (so the neighbours of an entry leave
    room for a duplicate and for a descent by one without a second violation); max 135 < COLS."""
    start = (3 * i) % 7 + 1
    return [start + 2 * k for k in range(n)]


def build(rows: int, forced=None, columns=_columns):
    """(indptr int64, indices int32) of the canonical base matrix."""
    lens = row_lengths(rows, forced)
    indptr = np.zeros(rows + 1, dtype=np.int64)
    indptr[1:] = np.cumsum(lens)
    cols = [c for i, n in enumerate(lens) for c in columns(i, n)]
    return indptr, np.asarray(cols, dtype=np.int32).reshape(-1)


def fault_rows(rows: int):
    """Rows 0, 255, 256 and the last one, as far as the matrix has them."""
    return sorted({r for r in (0, BLOCK - 1, BLOCK, rows - 1) if 0 <= r < rows})


def _frozen(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)


def _case(cid, rows, indptr, indices, expect, kind, at=(), repaired=None, cols=COLS):
    _frozen(indptr, indices, repaired)
    return Case(cid, rows, cols, indptr, indices, expect, kind, at, repaired)


@functools.lru_cache(maxsize=None)
def cases():
    """Every case, in a fixed order."""
    out = []
    # no rows at all; rows without a single entry (null indices and values on the device)
    out.append(_case("rows0", 0, np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32), 1, "canonical"))
    for rows in (1, BLOCK + 1):
        out.append(_case(f"r{rows}-nnz0", rows, np.zeros(rows + 1, dtype=np.int64), np.zeros(0, dtype=np.int32), 1,
                         "canonical"))
    for rows in ROW_COUNTS:
        last = rows - 1
        # the base: canonical rows of 0, 1, 2 and 65 entries, empty runs at both ends
        p, j = build(rows)
        out.append(_case(f"r{rows}-base", rows, p, j, 1, "canonical"))

        # exactly one order violation, repaired alongside
        for r in fault_rows(rows):
            p, j = build(rows, {r: LONG})
            for where, e in (("first", 1), ("last", LONG - 1)):
                q = int(p[r]) + e
                for name, value in (("dup", int(j[q - 1])), ("down1", int(j[q - 1]) - 1), ("to0", 0)):
                    bad = j.copy()
                    bad[q] = value
                    out.append(_case(f"r{rows}-order-{name}-{where}pair-row{r}", rows, p, bad, 0, "one_violation",
                                     (r, e), j.copy()))

        # the last column of a row >= the first column of the next non-empty row, everywhere: no violation
        forced = {BLOCK - 1: 2, BLOCK: 2} if rows > BLOCK else {}
        p, j = build(rows, forced, lambda i, n: [1] if n == 1 else [2 * k for k in range(n)])
        out.append(_case(f"r{rows}-drop-across-rows", rows, p, j, 1, "row_boundary_drops"))

        # a row of one entry in column 0 (prev starts at -1) and one in column cols - 1 (the >= cols bound)
        for name, r, c in (("col0", 0, 0), ("colmax", last, COLS - 1)):
            p, j = build(rows, {r: 1})
            j = j.copy()
            j[int(p[r])] = c
            out.append(_case(f"r{rows}-single-{name}-row{r}", rows, p, j, 1, "single_entry_row", (r, c)))

        # one index out of range: the first entry of row 0, the last entry of the last row
        for name, value in (("minus1", -1), ("cols", COLS), ("int32max", INT32_MAX)):
            for where, r, e in (("first", 0, 0), ("last", last, LONG - 1)):
                p, j = build(rows, {r: LONG})
                bad = j.copy()
                bad[int(p[r]) + e] = value
                out.append(_case(f"r{rows}-index-{name}-{where}", rows, p, bad, -1, "one_bad_index", (r, e)))

        # an order violation in row 0 and a bad index in the last row (one row: both in it): -1 wins
        p, j = build(rows, {0: LONG, last: LONG})
        bad = j.copy()
        bad[int(p[0]) + 1] = bad[int(p[0])]
        bad[int(p[last]) + LONG - 1] = COLS
        out.append(_case(f"r{rows}-order-and-index", rows, p, bad, -1, "violation_and_bad_index"))

        # bad row pointers: only the values of indptr change
        p, j = build(rows, {0: LONG, last: LONG})
        nnz, mid = int(j.size), rows // 2
        for name, k, value in (("negative-first", 0, -1), ("negative-mid", mid, -1),
                               ("last-nnz-plus-1", rows, nnz + 1), ("interior-above-nnz", mid, nnz + 5),
                               ("decreasing-mid", mid, None)):
            if name.endswith(("-mid", "interior-above-nnz")) and rows < 3:
                continue                       # no interior entry
            q = p.copy()
            if value is None:                  # indptr[mid] one past indptr[mid + 1]: row mid ends before it starts
                value = int(p[mid + 1]) + 1
                assert value <= nnz
            q[k] = value
            out.append(_case(f"r{rows}-indptr-{name}", rows, q, j.copy(), -1, "bad_indptr", (k,)))
        if rows == 1:                          # the one row ends before it starts
            out.append(_case("r1-indptr-decreasing", 1, np.asarray([nnz, 0], dtype=np.int64), j.copy(), -1,
                             "bad_indptr", (0,)))
    ids = [c.id for c in out]
    assert len(set(ids)) == len(ids)
    return tuple(out)


def by_id(cid: str) -> Case:
    return next(c for c in cases() if c.id == cid)


def repaired_cases():
    return tuple(c for c in cases() if c.repaired is not None)


# the verdicts one handle gives in a row (tests/test_gpu_validate.py): -1, 1, 0, 1, -1, 1
SEQUENCE = ("r257-index-int32max-last", "r513-base", "r257-order-dup-lastpair-row256", "r1-base",
            "r513-indptr-negative-mid", "r256-drop-across-rows")
SEQUENCE_VERDICTS = (-1, 1, 0, 1, -1, 1)
# the cases run with every value type
CANONICAL_ID, VIOLATING_ID = "r257-base", "r257-order-down1-firstpair-row256"
