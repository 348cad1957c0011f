"""Inputs that put the rows of a CSR matrix on the seams of the dense-operand kernels (k_spmv,
k_spmm_col, k_spmm_row, k_spmm_row_packed), shared by tests/test_dense_seams_cpu.py and
tests/test_gpu_dense_seams.py.  A plain helper module (no pytest hooks); everything is generated
from seeds.

k_spmv and k_spmm_col give a wave 64 consecutive rows (a GROUP here) and stage the group's
contiguous entry range through LDS in chunks of `ch` entries counted from the group's first
entry: SPMV_CH = 1024 for k_spmv, SPMM_CH = 512 for k_spmm_col.  A block holds 4 waves.
seam_matrix(ch, dtype) has 728 rows and 4096 columns: eleven groups of 64 rows and one ragged
group of 24, so three full blocks of four waves, the ragged group being the fourth wave of the
last one.  No wave of it leaves early; the row-count matrices reach that.  T is a group's entry
total and L = 2 * ch + 452 the length of a long row:

  empty       T = 0
  one         T = 1, the entry in the group's last row
  ch-1, ch    T = ch - 1 and T = ch, spread evenly
  ch+1        rows 0..62 hold ch entries in all, row 63 holds one, alone in the second chunk
  2ch         rows 0..30 hold exactly ch, row 31 is empty and sits on the chunk boundary, rows
              32..63 hold ch
  straddle    T = 2 * ch + 1: rows 0..9 hold ch - 32, row 10 holds 65 and crosses the first
              boundary, the rest is spread evenly
  long-first, long-last, long-mid
              one row of L entries (three chunks or more) at lane 0, at lane 63, and at lane 31
              between two empty rows; the other rows hold 0..8
  random      rows of 0..40
  ragged      23 rows of 0..40, then a last row of 130
"""
from __future__ import annotations

import functools

import numpy as np
import scipy.sparse as sp

from tests.instantiations import DTYPES, seed_of

SPMV_CH, SPMM_CH = 1024, 512          # spgemm_spmv.hpp, spgemm_spmm.hpp
WAVE, WPB = 64, 4
COLS = 4096
GROUPS = ["empty", "one", "ch-1", "ch", "ch+1", "2ch", "straddle", "long-first", "long-last", "long-mid",
          "random", "ragged"]
RAGGED_ROWS = 24
ROWS = (len(GROUPS) - 1) * WAVE + RAGGED_ROWS    # 728
LONG_LANE = {"long-first": 0, "long-last": 63, "long-mid": 31}
ROW_COUNTS = [1, 63, 64, 65, 255, 256, 257]
# k_spmm_row / k_spmm_row_packed: each side of the 64-entry batch, of spmm_walk's 8-entry unroll
# and of the packed kernel's 4-entry unroll
ROW_MAJOR_LENGTHS = [0, 1, 3, 4, 5, 7, 8, 9, 63, 64, 65, 71, 72, 73, 127, 128, 129, 200]
ROW_MAJOR_ROWS, ROW_MAJOR_COLS = 71, 256


def long_len(ch):
    return 2 * ch + 452


def group_start(name):
    """First row of a group."""
    return GROUPS.index(name) * WAVE


def _spread(total, rows):
    """`total` entries over `rows` rows as evenly as possible (the first rows take the rest)."""
    base, extra = divmod(total, rows)
    return [base + (1 if i < extra else 0) for i in range(rows)]


def group_lengths(name, ch, rng):
    """Row lengths of one group."""
    if name == "empty":
        return [0] * WAVE
    if name == "one":
        return [0] * (WAVE - 1) + [1]
    if name == "ch-1":
        return _spread(ch - 1, WAVE)
    if name == "ch":
        return _spread(ch, WAVE)
    if name == "ch+1":
        return _spread(ch, WAVE - 1) + [1]
    if name == "2ch":
        return _spread(ch, 31) + [0] + _spread(ch, 32)
    if name == "straddle":
        return _spread(ch - 32, 10) + [65] + _spread(2 * ch + 1 - (ch - 32) - 65, WAVE - 11)
    if name in LONG_LANE:
        lens = [int(v) for v in rng.integers(0, 9, WAVE)]
        lane = LONG_LANE[name]
        lens[lane] = long_len(ch)
        if name == "long-mid":
            lens[lane - 1] = lens[lane + 1] = 0
        return lens
    if name == "random":
        return [int(v) for v in rng.integers(0, 41, WAVE)]
    if name == "ragged":
        return [int(v) for v in rng.integers(0, 41, RAGGED_ROWS - 1)] + [130]
    raise KeyError(name)


def _values(rng, shape, dt):
    v = rng.standard_normal(shape)
    if np.dtype(dt).kind == "c":
        v = v + 1j * rng.standard_normal(shape)
    return v.astype(dt)


def dense_values(seed, shape, dtype):
    """standard_normal values (complex: both parts) of a dense operand, read-only."""
    v = _values(np.random.default_rng(seed_of("dense_seams", seed, shape, np.dtype(dtype).name)), shape, dtype)
    v.setflags(write=False)
    return v


def _from_lengths(lens, cols, rng, dt):
    lens = np.asarray(lens, dtype=np.int64)
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    indices = (np.concatenate([np.sort(rng.choice(cols, int(m), replace=False)) for m in lens]).astype(np.int32)
               if lens.sum() else np.zeros(0, np.int32))
    A = sp.csr_matrix((_values(rng, int(lens.sum()), dt), indices, indptr), shape=(len(lens), cols))
    assert A.has_canonical_format
    for a in (A.data, A.indices, A.indptr):
        a.setflags(write=False)
    return A


@functools.lru_cache(maxsize=None)
def _seam_matrix(ch, dname):
    rng = np.random.default_rng(seed_of("seam_matrix", ch, dname))
    lens = [m for g in GROUPS for m in group_lengths(g, ch, rng)]
    assert len(lens) == ROWS
    return _from_lengths(lens, COLS, rng, DTYPES[dname])


def _dname(dtype):
    return dtype if isinstance(dtype, str) else {np.dtype(v): k for k, v in DTYPES.items()}[np.dtype(dtype)]


def seam_matrix(ch, dtype):
    """The 728 x 4096 canonical CSR matrix described in the module docstring for chunk size `ch`
    (generated once per (ch, dtype), read-only).  dtype: a numpy dtype or "f32" / "f64" / "c64" /
    "c128"."""
    return _seam_matrix(int(ch), _dname(dtype))


@functools.lru_cache(maxsize=None)
def _row_count_matrix(rows, dname):
    rng = np.random.default_rng(seed_of("row_count", rows, dname))
    return _from_lengths(rng.integers(0, 13, rows), 257, rng, DTYPES[dname])


def row_count_matrix(rows, dtype):
    """rows x 257 with row lengths 0..12: the ragged wave (rows % 64) and the waves of a block
    that leave at once (rows <= 192 in the last block of 256)."""
    return _row_count_matrix(int(rows), _dname(dtype))


@functools.lru_cache(maxsize=None)
def _row_major_matrix(dname):
    rng = np.random.default_rng(seed_of("row_major", dname))
    lens = (ROW_MAJOR_LENGTHS * 4)[:ROW_MAJOR_ROWS]
    return _from_lengths(lens, ROW_MAJOR_COLS, rng, DTYPES[dname])


def row_major_matrix(dtype):
    """71 x 256, the row lengths ROW_MAJOR_LENGTHS repeated to fill; 71 is odd, so every
    rows-per-wave of k_spmm_row_packed ends ragged."""
    return _row_major_matrix(_dname(dtype))


def beta_of(dtype):
    """The beta != 0 of the epilogue cases (complex for complex types)."""
    return (0.25 + 0.5j) if _dname(dtype).startswith("c") else 0.25
