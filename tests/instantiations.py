"""Every compiled kernel instantiation at its structural edges: the case table, the inputs with
hand-placed edge rows, the planner's rules restated in Python and the C-ABI driver shared by
tests/test_instantiations_cpu.py and tests/test_gpu_instantiations.py.

A plain helper module (no pytest hooks).  Everything is generated from seeds.

The C-ABI driver (run_abi, run_ws, run_tiles) hands the library poisoned, guarded buffers
(tests/guarded.py) for everything it writes -- the workspace at exactly its queried size and C's
three arrays -- checks the guard bands after the final synchronize and compares A's and B's device
arrays with what was uploaded; run_poisoned is the per-case schedule of
tests/test_gpu_poisoned_products.py (both poisons, repeated spg_symbolic, a stale shared
workspace, ALG1's workspace hand-off, spg_spgemm_ws).

What the other parity tests leave out: they reach most kernels with random matrices of int32 row
pointers and moderate row lengths.  Here every case runs with A/B row pointers (IP) and C row
pointers (CP) of both widths -- the C ABI lets the caller choose C's, where the Python shim picks
it from nnz(C) -- under ALG1, ALG2 and chunked ALG3, on inputs whose rows sit exactly on the
kernels' seams:

  A row lengths (tile and general cases), NB = 4 for complex128 and 8 otherwise (the register
  queue of dn_fetch / k_tile preloads NB batches of 64 A entries; later batches load through
  another branch): 0, 1, 63, 64, 65, 127, 128, 129, NB*64 - 1, NB*64, NB*64 + 1, (NB + 1)*64,
  2*NB*64 + 1.  The first row (2*NB*64 + 1) and the last row (NB*64 + 1) of A are edge rows, and
  the (NB + 1)*64 row stands between two empty rows.

  Special B rows (tile cases), one set for an inner tile g = 1 and one for the ragged last tile,
  both sets at both ends of B's row range (rows 0.. and ..k - 1, so that A's sorted columns put
  them first or last in a row): empty; one entry at the tile's first column; one at its last;
  both plus the first column of the next tile (last tile: plus the last column of the tile
  before); one entry at column n - 1; the whole tile (twice, with different values); 63, 64 and
  65 entries inside the tile; on sparse tiles the first CAP columns of the tile (CAP: a window's
  slot count) and a row holding only the next column.  A rows combine them: the full row alone,
  the CAP row alone, CAP row + next column, two different full rows, every special row of one
  end, only the empty row, and the seam row: NB*64 + 1 entries whose entries 0, 63, 64,
  NB*64 - 1 and NB*64 are one-entry (entry 0: three-entry) special rows that all hit the inner
  tile's first or last column, so the entry on each side of a batch seam and of the queue seam
  takes part in an ordered sum.

  Record groups (sparse8192): 40000 columns are 5 tiles of 8192, so the one group of 8 has three
  padding tiles; one A row of NB*64 + 1 entries has products only in the last real tile.

  Short case (spgemm_row.hpp: RowSmall, R = 10 chunks of 64 products, PREG = 640, LCAP = 64,
  NW = 512): rows of 63, 64 and 65 entries (65 spills); rows of 128/129, 256/257, 384/385,
  512/513, 640 products (each side of a chunk-count variant of row_dispatch) and 641 (spills); a
  row whose products in flagged bitmap words number exactly LCAP and one with LCAP + 1 (spills);
  the 640-product row has 640 distinct output columns, more than one stage window of
  row_write_staged (W = offsetof(RowLds, lb_gw) / (sizeof(T) + 4): fp64 517 with int32 row
  pointers and 602 with int64, complex64 the same, complex128 387; fp32 776 / 904, which no row
  of <= 640 products can exceed), and touches columns 0 and n - 1.  short64 is the same structure
  without the 65-entry row: k_short's single pass (ALG1) refuses that row and no other, so only
  there does the C it writes stay.

Planner margins (plan(): value / threshold of every inequality that decides a case, measured on
the generated inputs; test_instantiations_cpu.py asserts each is at least MARGIN away from 1):
  short-f32:
      short: avgA <= 48: 10.22 / 48 = 0.21
      short: avgA*avgB <= 400: 79.52 / 400 = 0.20
  short-f64, short-kshort-f64:
      short: avgA <= 48: 10.14 / 48 = 0.21
      short: avgA*avgB <= 400: 78.97 / 400 = 0.20
  short64-kshort-f64:
      short: avgA <= 48: 9.761 / 48 = 0.20
      short: avgA*avgB <= 400: 75.98 / 400 = 0.19
  short-c64:
      short: avgA <= 48: 10.05 / 48 = 0.21
      short: avgA*avgB <= 400: 78.23 / 400 = 0.20
  short-c128:
      short: avgA <= 48: 10.49 / 48 = 0.22
      short: avgA*avgB <= 400: 81.68 / 400 = 0.20
  general-f32:
      width loop: frac*2048 <= 0.95*1024: 26.05 / 972.8 = 0.03
      width loop: frac*4096 <= 0.95*1024: 52.09 / 972.8 = 0.05
      tile path: frac*4096 >= 64: 52.09 / 64 = 0.81
  general-f64:
      width loop: frac*2048 <= 0.95*1024: 26.05 / 972.8 = 0.03
      width loop: frac*4096 <= 0.95*1024: 52.1 / 972.8 = 0.05
      sparse 8192: frac >= 0.1: 0.01272 / 0.1 = 0.13
      sparse 8192: frac*8192 <= 0.95*2048: 104.2 / 1946 = 0.05
      tile path: frac*4096 >= 64: 52.1 / 64 = 0.81
  general-c64, general-c128:
      width loop: frac*2048 <= 0.95*1024: 26.05 / 972.8 = 0.03
      width loop: frac*4096 <= 0.95*1024: 52.1 / 972.8 = 0.05
      tile path: frac*4096 >= 64: 52.1 / 64 = 0.81
  owner-sparse-f32:
      not short: max(avgA/48, avgA*avgB/400) > 1: 5.741 / 1 = 5.74
      width loop: frac*2048 <= 0.95*1024: 689.3 / 972.8 = 0.71
      width loop: frac*4096 <= 0.95*1024: 1379 / 972.8 = 1.42
      tile path: frac*2048 >= 64: 689.3 / 64 = 10.77
      symbolic: widest segment >= 128: 56.01 / 128 = 0.44
  owner-sparse-c64:
      not short: max(avgA/48, avgA*avgB/400) > 1: 5.739 / 1 = 5.74
      width loop: frac*2048 <= 0.95*1024: 689.1 / 972.8 = 0.71
      width loop: frac*4096 <= 0.95*1024: 1378 / 972.8 = 1.42
      tile path: frac*2048 >= 64: 689.1 / 64 = 10.77
      symbolic: widest segment >= 128: 55.99 / 128 = 0.44
  owner-dense-f32, runs32-f32:
      not short: max(avgA/48, avgA*avgB/400) > 1: 505.8 / 1 = 505.77
      width loop: frac*2048 <= 0.95*1024: 2048 / 972.8 = 2.11
      width loop: frac*4096 <= 0.95*1024: 4096 / 972.8 = 4.21
      tile path: frac*1024 >= 64: 1024 / 64 = 16.00
      symbolic: widest segment >= 128: 493.4 / 128 = 3.85
      fp32 runs: segment >= 48: 202.1 / 48 = 4.21
  owner-dense-c64:
      not short: max(avgA/48, avgA*avgB/400) > 1: 505.8 / 1 = 505.85
      width loop: frac*2048 <= 0.95*1024: 2048 / 972.8 = 2.11
      width loop: frac*4096 <= 0.95*1024: 4096 / 972.8 = 4.21
      tile path: frac*1024 >= 64: 1024 / 64 = 16.00
      symbolic: widest segment >= 128: 493.5 / 128 = 3.86
  dense1024-f64, dense1024-c128:
      not short: max(avgA/48, avgA*avgB/400) > 1: 18.86 / 1 = 18.86
      width loop: frac*2048 <= 0.95*1024: 1651 / 972.8 = 1.70
      width loop: frac*4096 <= 0.95*1024: 3302 / 972.8 = 3.39
      tile path: frac*1024 >= 64: 825.6 / 64 = 12.90
      symbolic: widest segment >= 128: 91.98 / 128 = 0.72
  dense2048-f64:
      width loop: frac*2048 <= 0.95*1024: 1674 / 972.8 = 1.72
      width loop: frac*4096 <= 0.95*1024: 3348 / 972.8 = 3.44
      dense 2048: frac >= 0.5: 0.8173 / 0.5 = 1.63
      tile path: frac*2048 >= 64: 1674 / 64 = 26.15
      symbolic: widest segment >= 128: 170 / 128 = 1.33
  sparse4096-f64, sparse4096-c128:
      not short: max(avgA/48, avgA*avgB/400) > 1: 5.025 / 1 = 5.02
      width loop: frac*2048 <= 0.95*1024: 372.9 / 972.8 = 0.38
      width loop: frac*4096 <= 0.95*1024: 745.8 / 972.8 = 0.77
      tile path: frac*4096 >= 64: 745.8 / 64 = 11.65
      symbolic: widest segment >= 128: 67 / 128 = 0.52
  sparse8192-f64, sparse8192-f64-rg1:
      width loop: frac*2048 <= 0.95*1024: 412.4 / 972.8 = 0.42
      width loop: frac*4096 <= 0.95*1024: 824.9 / 972.8 = 0.85
      sparse 8192: frac >= 0.1: 0.2014 / 0.1 = 2.01
      sparse 8192: frac*8192 <= 0.95*2048: 1650 / 1946 = 0.85
      tile path: frac*8192 >= 64: 1650 / 64 = 25.78
      symbolic: widest segment >= 128: 149.9 / 128 = 1.17
"""
from __future__ import annotations

import contextlib
import ctypes
import functools
import math
import os
import zlib
from collections import namedtuple

import numpy as np
import scipy.sparse as sp

DTYPES = {"f32": np.float32, "f64": np.float64, "c64": np.complex64, "c128": np.complex128}
VALUE_TYPE = {"f32": 0, "f64": 1, "c64": 4, "c128": 5}        # spg_dtype_t
ROWS = 176                                                     # rows of every case's A
MARGIN = 0.03
WIDTHS = [(32, 32), (32, 64), (64, 32), (64, 64)]              # (IP, CP)
ALGS = [1, 2, "3c"]
CF = 0.1                                                       # chunk_fraction: >= 10 chunks under "3c"

# spgemm_row.hpp, RowSmall
ROW_ENTRIES, ROW_PREG, ROW_LCAP, ROW_NW = 64, 640, 64, 512
# spgemm_tile.hpp / spgemm_tile_dn.hpp
TILE_CAP, DN_TW_MAX, SEG_MIN, F32_RUN_MIN = 1024, 2048, 128.0, 48.0


def nb_of(dname):
    """Batches of 64 A entries the tile kernels preload (dn_fetch, k_tile_sp, k_tile)."""
    return 4 if np.dtype(DTYPES[dname]).itemsize > 8 else 8


def a_lengths(dname):
    q = nb_of(dname) * 64
    return [0, 1, 63, 64, 65, 127, 128, 129, q - 1, q, q + 1, q + 64, 2 * q + 1]


# ---------------------------------------------------------------------------------------------
# Structures: name -> kind, k, n, entries per row of A and of B (the planner sees only these
# averages and n), tile width, window capacities of the sparse-tile kernels that may run on it,
# record-group case.  Densities are those of special_values.STRUCTS where a structure exists
# there; n is moved off the tile multiple so that the last tile is ragged.
#   general: 64 entries per A row (special_values has 75 for its `ints` floor, 5 % under the tile
#            path's threshold; the margin here is 19 %).
#   sparse4096: under 16384 columns, so fp64 stays on 4096-column tiles whatever frac is.
#   sparse4096, sparse8192: few entries per A row and many per B row at the product the planner
#            needs (avgA * avgB / n = 0.2 and 0.225), so that the long edge rows, whose C rows are
#            dense, carry most of the products: 20 % of C's entries must sum two or more products,
#            and random rows at these expected densities alone give 10 %.
Struct = namedtuple("Struct", "kind k n avg_a avg_b tw caps rg")
STRUCTS = {
    "short": Struct("short", 2048, 2048, 8.0, 8.0, 0, (), False),
    # `short` without its 65-entry A row (an ordinary fill row in its place): no row k_short's
    # single pass refuses (it takes rows of <= 64 entries whatever their products)
    "short64": Struct("short", 2048, 2048, 8.0, 8.0, 0, (), False),
    "general": Struct("general", 2000, 200000, 64.0, 40.0, 4096, (), False),
    "owner": Struct("tile", 4096, 5596, 41.0, 56.0, 2048, (1024,), False),
    "runs32": Struct("tile", 2048, 2500, 410.0, 500.0, 1024, (), False),
    "dense1024": Struct("tile", 4096, 4596, 82.0, 92.0, 1024, (), False),
    "dense2048": Struct("tile", 17000, 17000, 170.0, 170.0, 2048, (), False),
    "sparse4096": Struct("tile", 4096, 10000, 30.0, 67.0, 4096, (1024,), False),
    "sparse8192": Struct("tile", 8000, 40000, 60.0, 150.0, 8192, (2032, 2048), True),
}

# The case table: (id, structure, dtype, env, expect, kernel, symbolic kernel).  `expect` is what
# plan_info must say; `kernel` is the numeric kernel that then runs (spgemm.hip tile_numeric /
# the short and general drivers); the symbolic kernel follows from sym_tile_log2: k_tile_sym_seg
# when the widest symbolic tile holds B segments of >= 128 entries (runs32: 500, dense2048: 170,
# sparse8192: 150), k_tile_sym8c otherwise (owner 56, dense1024 92, sparse4096 67).  So each of the
# two runs with bitmaps (sparse tiles) and without (dense tiles take their structure from the
# accumulation; their symbolic pass still counts with that kernel).
Case = namedtuple("Case", "id struct dname env expect kernel sym")
_T = "tile"


def _tile(tw, dense, ordered, rg=1):
    return {"path": _T, "tile_width": tw, "dense_tiles": dense, "lds_ordered": ordered, "record_group": rg}


CASES = (
    [Case(f"short-{d}", "short", d, {}, {"path": "short"}, "k_row (+ k_symbolic / k_numeric on spilled rows)", None)
     for d in DTYPES] +
    [Case("short-kshort-f64", "short", "f64", {"SPG_SHORT_KERNEL": "short"}, {"path": "short"}, "k_short", None),
     Case("short64-kshort-f64", "short64", "f64", {"SPG_SHORT_KERNEL": "short"}, {"path": "short"},
          "k_short (ALG1: the single pass holds)", None)] +
    [Case(f"general-{d}", "general", d, {}, {"path": "general"}, "k_symbolic / k_numeric", None) for d in DTYPES] +
    [Case(f"owner-sparse-{d}", "owner", d, {}, _tile(2048, False, False), "k_tile<T, DENSE=0>", "k_tile_sym8c")
     for d in ("f32", "c64")] +
    [Case("owner-dense-f32", "runs32", "f32", {"SPG_F32_RUNS": "0"}, _tile(1024, True, False),
          "k_tile<float, DENSE=1>", "k_tile_sym_seg"),
     Case("owner-dense-c64", "runs32", "c64", {}, _tile(1024, True, False), "k_tile<complex64, DENSE=1>",
          "k_tile_sym_seg"),
     Case("runs32-f32", "runs32", "f32", {}, _tile(1024, True, True), "k_tile_dn<float, 1024>", "k_tile_sym_seg"),
     Case("dense1024-f64", "dense1024", "f64", {}, _tile(1024, True, True), "k_tile_dn<double, 1024>", "k_tile_sym8c"),
     Case("dense1024-c128", "dense1024", "c128", {}, _tile(1024, True, True), "k_tile_dn<complex128, 1024>",
          "k_tile_sym8c"),
     Case("dense2048-f64", "dense2048", "f64", {}, _tile(2048, True, True), "k_tile_dn<double, 2048>", "k_tile_sym_seg"),
     Case("sparse4096-f64", "sparse4096", "f64", {}, _tile(4096, False, True), "k_tile_sp<double, SpCfg1024, 1>",
          "k_tile_sym8c"),
     Case("sparse4096-c128", "sparse4096", "c128", {}, _tile(4096, False, True), "k_tile_sp<complex128, SpCfg1024, 1>",
          "k_tile_sym8c"),
     Case("sparse8192-f64", "sparse8192", "f64", {}, _tile(8192, False, True, 8), "k_tile_sp<double, SpCfgRG, 8>",
          "k_tile_sym_seg"),
     Case("sparse8192-f64-rg1", "sparse8192", "f64", {"SPG_SP_RECORD_GROUP": "1"}, _tile(8192, False, True, 1),
          "k_tile_sp<double, SpCfg2048, 1>", "k_tile_sym_seg")])
CASE = {c.id: c for c in CASES}
CASE_IDS = [c.id for c in CASES]
# SPG_SHORT_KERNEL is read once per process: such a case runs in a child process
CHILD_ENV = ("SPG_SHORT_KERNEL",)


def seed_of(*parts):
    return zlib.crc32("|".join(str(p) for p in parts).encode())


# ---------------------------------------------------------------------------------------------
# The planner, restated from spgemm.hip (want_short, want_tile, tile_dense, sym_tile_log2,
# fp32_runs, record_group_log2, spg_plan_info).  `lean` / `lean32`: the handle's LDS checks
# passed, as they do on gfx950.

def plan(rows_a, nnz_a, k, nnz_b, n, dname, env=None, lean=True, lean32=True):
    """What spg_plan decides from the averages, and the margin of every inequality that decided:
    margins is a list of (name, value, threshold); value / threshold is compared with 1."""
    env = env or {}
    avg_a, avg_b = nnz_a / rows_a, nnz_b / k
    mg = []
    out = {"path": "general", "tile_width": 0, "dense_tiles": False, "lds_ordered": False, "record_group": 0,
           "sym": None, "margins": mg}
    if n <= 32 * ROW_NW:
        if avg_a <= 48.0 and avg_a * avg_b <= 400.0:
            mg += [("short: avgA <= 48", avg_a, 48.0), ("short: avgA*avgB <= 400", avg_a * avg_b, 400.0)]
            out["path"] = "short"
            return out
        # (either condition failing keeps a shape off the short path: the larger excess decides)
        mg.append(("not short: max(avgA/48, avgA*avgB/400) > 1", max(avg_a / 48.0, avg_a * avg_b / 400.0), 1.0))
    frac = 1.0 - math.exp(-avg_a * avg_b / n)
    tws = 8
    for t in range(8, 13):
        tw = float(1 << t)
        if tw > TILE_CAP:
            mg.append((f"width loop: frac*{1 << t} <= 0.95*1024", frac * tw, 0.95 * TILE_CAP))
        if tw <= TILE_CAP or frac * tw <= 0.95 * TILE_CAP:
            tws = t
        if tw >= n:
            break
    f64 = dname == "f64"
    if f64 and lean and tws == 10 and n >= 16384:
        mg.append(("dense 2048: frac >= 0.5", frac, 0.5))
        if frac >= 0.5:
            tws = 11
    if f64 and lean and tws == 12 and n >= 16384:
        mg += [("sparse 8192: frac >= 0.1", frac, 0.1), ("sparse 8192: frac*8192 <= 0.95*2048", frac * 8192, 0.95 * 2048)]
        if frac >= 0.1 and frac * 8192.0 <= 0.95 * 2048:
            tws = 13
    mg.append((f"tile path: frac*{1 << tws} >= 64", frac * (1 << tws), 64.0))
    if frac * (1 << tws) < 64.0:
        return out
    out["path"] = "tile"
    out["tile_width"] = 1 << tws
    out["tiles_per_row"] = (n + (1 << tws) - 1) >> tws
    cap = DN_TW_MAX if (f64 and lean) else TILE_CAP
    dense = (1 << tws) <= cap
    out["dense_tiles"] = dense
    # sym_tile_log2
    tmax = tws
    while tmax < 16 and (1 << tmax) < n:
        tmax += 1
    seg_max = avg_b * min(1.0, (1 << tmax) / n)
    mg.append(("symbolic: widest segment >= 128", seg_max, SEG_MIN))
    out["sym"] = "k_tile_sym_seg" if seg_max >= SEG_MIN else "k_tile_sym8c"
    # fp32_runs
    runs = False
    if dname == "f32" and lean32 and (1 << tws) <= 1024:
        seg = avg_b * (1 << tws) / n
        mg.append(("fp32 runs: segment >= 48", seg, F32_RUN_MIN))
        runs = seg >= F32_RUN_MIN and env.get("SPG_F32_RUNS") != "0"
    out["lds_ordered"] = bool(lean and dname in ("f64", "c128")) or (dense and runs)
    rg = 1
    if not dense and lean and f64 and tws == 13 and env.get("SPG_SP_RECORD_GROUP") != "1":
        rg = 8
    out["record_group"] = rg
    return out


def plan_case(case):
    c = CASE[case]
    A, B, _ = inputs(case)
    return plan(A.shape[0], A.nnz, B.shape[0], B.nnz, B.shape[1], c.dname, c.env)


# ---------------------------------------------------------------------------------------------
# Inputs

def _values(rng, nnz, dt):
    v = rng.standard_normal(nnz)
    if np.dtype(dt).kind == "c":
        v = v + 1j * rng.standard_normal(nnz)
    return v.astype(dt)


def _csr(rows, shape, rng, dt):
    """Canonical CSR from a list of sorted, duplicate-free column arrays, standard_normal values."""
    lens = np.array([len(r) for r in rows], dtype=np.int64)
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    indices = (np.concatenate([np.asarray(r, dtype=np.int32) for r in rows]) if lens.sum() else np.zeros(0, np.int32))
    M = sp.csr_matrix((_values(rng, int(lens.sum()), dt), indices.astype(np.int32), indptr), shape=shape)
    assert M.has_canonical_format
    return M


def _random_rows(rng, rows, n, total, lo=0):
    """{row: sorted distinct columns in [lo, n)} for `rows`, about `total` entries in all (random
    (row, column) pairs with duplicates dropped), no row empty."""
    rows = np.asarray(rows)
    r = rng.integers(0, len(rows), max(int(total), 0))
    c = rng.integers(lo, n, max(int(total), 0))
    key = np.unique(r.astype(np.int64) * n + c)
    r, c = key // n, key % n
    cuts = np.searchsorted(r, np.arange(len(rows) + 1))
    out = {}
    for i, row in enumerate(rows):
        cols = c[cuts[i]:cuts[i + 1]]
        out[int(row)] = cols if len(cols) else np.array([int(rng.integers(lo, n))])
    return out


def _tile_specials(rng, n, c0, w, caps, last, small):
    """The special B rows of one tile [c0, c0 + w): a list of (label, columns)."""
    sub = lambda m: c0 + np.sort(rng.choice(w, m, replace=False))
    rows = [("empty", []), ("first", [c0]), ("last", [c0 + w - 1]),
            ("straddle", [c0 - 1, c0, c0 + w - 1] if last else [c0, c0 + w - 1, c0 + w]),
            ("nminus1", [n - 1]), ("e63", sub(63)), ("e64", sub(64)), ("e65", sub(65))]
    if not small:
        rows += [("full", np.arange(c0, c0 + w)), ("full2", np.arange(c0, c0 + w))]
        for cap in caps:
            assert w > cap, (w, cap)   # the ragged tile is wide enough for a full window plus one
            rows += [(f"cap{cap}", np.arange(c0, c0 + cap)), (f"capnext{cap}", [c0 + cap])]
    return rows


Meta = namedtuple("Meta", "edge special items spill")
# edge: {label: A row}; special: {label: B row}; items: [(A row, column lo, column hi, nnz)] the
# entry counts the oracle's C must show; spill: short case, {label: (entries, products, flagged
# products, distinct columns, taken)}.


@functools.lru_cache(maxsize=4)
def _inputs(struct, dname):
    S = STRUCTS[struct]
    rng = np.random.default_rng(seed_of("instantiations", struct, dname))
    if S.kind == "short":
        A, B, meta = _short_inputs(S, dname, rng, len65=struct != "short64")
    else:
        A, B, meta = _wide_inputs(S, dname, rng)
    for M in (A, B):
        for a in (M.data, M.indices, M.indptr):
            a.setflags(write=False)
    return A, B, meta


def inputs(case):
    """(A, B, meta) of a case; cases that differ only in their switches share their inputs."""
    return _inputs(CASE[case].struct, CASE[case].dname)


def _wide_inputs(S, dname, rng):
    dt = DTYPES[dname]
    k, n, tw = S.k, S.n, S.tw
    q = nb_of(dname) * 64
    small = S.kind == "general"
    G = (n + tw - 1) // tw
    assert G >= 3
    tiles = [("g", 1, tw, False), ("l", G - 1, n - (G - 1) * tw, True)]   # inner tile 1, ragged last tile
    assert 65 <= tiles[1][2] < tw
    # B: both sets of special rows at both ends, two one-entry rows in the middle, the rest random
    brow, special = {}, {}
    for end in ("lo", "hi"):
        block = [(f"{end}.{t}.{lab}", cols) for t, g, w, last in tiles
                 for lab, cols in _tile_specials(rng, n, g * tw, w, S.caps, last, small)]
        base = 0 if end == "lo" else k - len(block)
        for i, (lab, cols) in enumerate(block):
            special[lab], brow[base + i] = base + i, np.asarray(cols, dtype=np.int64)
    nblock = len(block)
    mid = k // 2
    special["mid.first"], brow[mid] = mid, np.array([tw])
    special["mid.last"], brow[mid + 1] = mid + 1, np.array([2 * tw - 1])
    lastrows = list(range(mid + 2, mid + 2 + q + 1)) if S.rg else []
    taken = set(brow) | set(lastrows)
    ordinary = np.array([r for r in range(k) if r not in taken])
    placed = sum(len(c) for c in brow.values())
    per = (S.avg_b * k - placed) / (len(ordinary) + len(lastrows))
    assert per >= 4, per
    brow.update(_random_rows(rng, ordinary, n, per * len(ordinary) * (1 + per / (2 * n))))
    if lastrows:   # rows with entries only in the last real tile
        brow.update(_random_rows(rng, lastrows, n, per * len(lastrows), lo=(G - 1) * tw))
    B = _csr([brow[r] for r in range(k)], (k, n), rng, dt)

    lo_ord, hi_ord = ordinary[ordinary < mid], ordinary[ordinary > mid + 1 + len(lastrows)]
    pick = lambda pool, m: np.sort(rng.choice(pool, m, replace=False))
    sp_ = lambda *labs: np.sort(np.array([special[x] for x in labs]))
    arow, edge, items = [], {}, []

    def put(label, cols):
        edge[label] = len(arow)
        arow.append(np.asarray(cols, dtype=np.int64))

    lens = a_lengths(dname)
    assert k - 2 * nblock - len(lastrows) - 2 > lens[-1]
    # the combination rows (all but the general case: it has no tiles)
    combos = []
    for t, g, w, last in ([] if small else tiles):
        c0 = g * tw
        combos.append((f"full.{t}", sp_(f"lo.{t}.full"), (c0, c0 + w, w)))
        combos.append((f"fullfull.{t}", sp_(f"lo.{t}.full", f"hi.{t}.full2"), (c0, c0 + w, w)))
        for cap in S.caps:
            combos.append((f"cap{cap}.{t}", sp_(f"hi.{t}.cap{cap}"), (c0, c0 + w, cap)))
            combos.append((f"cap{cap}+1.{t}", sp_(f"lo.{t}.cap{cap}", f"hi.{t}.capnext{cap}"), (c0, c0 + w, cap + 1)))
    for end in ("lo", "hi"):
        combos.append((f"all.{end}", sp_(*[x for x in special if x.startswith(end + ".") and
                                           x.rsplit(".", 1)[1] in ("empty", "first", "last", "straddle", "nminus1",
                                                                   "e63", "e64", "e65")]), None))
    combos.append(("onlyempty", sp_("lo.g.empty", "hi.l.empty"), (0, n, 0)))
    # the seam row: entries 0, 63, 64, q - 1 and q all hit column tw or 2 * tw - 1 of the inner tile
    seam = np.concatenate([sp_("lo.g.straddle"), pick(lo_ord, 62), sp_("mid.first", "mid.last"),
                           pick(hi_ord, q - 66), sp_("hi.g.first", "hi.g.last")])
    assert len(seam) == q + 1 and (np.diff(seam) > 0).all()
    combos.append(("seam", seam, None))
    if lastrows:
        combos.append(("lasttile", np.array(lastrows), ((G - 1) * tw, n, None)))

    def length_row(m):
        lab = f"len{m}"
        while lab in edge:
            lab += "'"
        put(lab, pick(ordinary, m))

    fillers = []

    def filler(m=1):
        for _ in range(m):
            fillers.append(len(arow))
            arow.append(None)

    length_row(lens[-1]); length_row(0); filler(2)            # first row: the longest
    for m in lens[1:8]:
        length_row(m); filler(3)
    length_row(lens[8]); length_row(lens[9]); filler(2)        # q - 1 and q side by side
    length_row(0); length_row(lens[11]); length_row(0)         # (NB + 1) * 64 between two empty rows
    filler(2)
    for lab, cols, item in combos:
        put(lab, cols)
        if item is not None:
            items.append((edge[lab], item[0], item[1], item[2]))
        filler(2)
    filler(ROWS - 1 - len(arow))
    length_row(lens[10])                                       # last row: q + 1
    assert len(arow) == ROWS
    rest = int(round(S.avg_a * ROWS)) - sum(len(r) for r in arow if r is not None)
    base, extra = divmod(rest, len(fillers))
    assert base >= 2, (rest, len(fillers))
    for i, r in enumerate(fillers):
        arow[r] = pick(ordinary, base + (1 if i < extra else 0))
    A = _csr(arow, (ROWS, k), rng, dt)
    return A, B, Meta(edge, special, items, None)


def row_stats(A, B, i):
    """(entries, products, products in flagged bitmap words, distinct columns) of C row i: the
    quantities k_row's spill rule looks at (a 32-column word is flagged once one of its columns
    is hit twice)."""
    js = A.indices[A.indptr[i]:A.indptr[i + 1]]
    cols = np.concatenate([B.indices[B.indptr[j]:B.indptr[j + 1]] for j in js]) if len(js) else np.zeros(0, np.int32)
    u, cnt = np.unique(cols, return_counts=True)
    flagged = np.unique(u[cnt > 1] >> 5)
    return len(js), len(cols), int(np.isin(cols >> 5, flagged).sum()), len(u)


def _short_inputs(S, dname, rng, len65=True):
    dt = DTYPES[dname]
    k, n = S.k, S.n
    w0, w1 = 40, 41                                   # the bitmap words of the flag rows
    free = np.array([c for c in range(1, n - 1) if (c >> 5) not in (w0, w1)])
    perm = rng.permutation(free)
    # pool of B rows with known lengths and pairwise distinct columns: 64 rows of 10 (the first
    # holds column 0, the last column n - 1), one of 11, 80 of 1
    take = iter(perm)
    nxt = lambda m: np.sort(np.array([next(take) for _ in range(m)]))
    p10 = [nxt(10) for _ in range(64)]
    p10[0] = np.sort(np.concatenate([[0], p10[0][1:]]))
    p10[63] = np.sort(np.concatenate([p10[63][:-1], [n - 1]]))
    p11, p1 = nxt(11), [nxt(1) for _ in range(80)]
    b0, b1 = 32 * w0, 32 * w1
    flag = [np.arange(b0, b0 + 16), np.concatenate([[b0], np.arange(b0 + 16, b0 + 31)]),
            np.arange(b1, b1 + 16), np.concatenate([[b1], np.arange(b1 + 16, b1 + 31)]), np.array([b0 + 31])]
    brow, special = {}, {}
    base = 100
    for lab, cols in ([(f"p10.{i}", c) for i, c in enumerate(p10)] + [("p11", p11)] +
                      [(f"p1.{i}", c) for i, c in enumerate(p1)] + [(f"flag{i}", c) for i, c in enumerate(flag)]):
        special[lab], brow[base] = base, cols
        base += 1
    special["empty"], brow[base] = base, np.zeros(0, np.int64)
    ordinary = np.array([r for r in range(k) if r not in brow])
    brow.update(_random_rows(rng, ordinary, n, S.avg_b * len(ordinary)))
    B = _csr([brow[r] for r in range(k)], (k, n), rng, dt)

    s10 = lambda m: [special[f"p10.{i}"] for i in range(m)]
    s1 = lambda m, off=0: [special[f"p1.{i}"] for i in range(off, off + m)]
    arow, edge = [], {}

    def put(label, cols):
        edge[label] = len(arow)
        arow.append(np.sort(np.asarray(cols, dtype=np.int64)))

    fill = lambda m=1: [arow.append(np.sort(rng.choice(ordinary, int(rng.integers(4, 11)), replace=False)))
                        for _ in range(m)]
    put("p640", s10(64)); put("len0", []); fill(2)             # first row: 64 entries, 640 products
    for P, (x, y) in {128: (12, 8), 129: (12, 9), 256: (25, 6), 257: (25, 7), 384: (38, 4), 385: (38, 5),
                      512: (51, 2), 513: (51, 3)}.items():
        put(f"p{P}", s10(x) + s1(y)); fill(2)
    put("p641", s10(63) + [special["p11"]]); fill(2)
    for m in (1, 63, 64, 65):
        if m == 65 and not len65:
            fill(1)                                            # (short64: an ordinary row in its place)
        else:
            put(f"len{m}", s1(m, 10))
        fill(2)
    put("flag64", [special[f"flag{i}"] for i in range(4)]); fill(2)
    put("flag65", [special[f"flag{i}"] for i in range(5)]); fill(2)
    put("onlyempty", [special["empty"]]); put("len0'", [])
    fill(ROWS - 1 - len(arow))
    put("p630+empty", s10(64)[1:] + [special["empty"]])       # last row: 64 entries, one of them an empty B row
    assert len(arow) == ROWS
    A = _csr(arow, (ROWS, k), rng, dt)
    spill = {}
    for lab, i in edge.items():
        e, P, L, nz = row_stats(A, B, i)
        spill[lab] = (e, P, L, nz, e <= ROW_ENTRIES and P <= ROW_PREG and L <= ROW_LCAP)
    return A, B, Meta(edge, special, [], spill)


@functools.lru_cache(maxsize=8)
def _reference(struct, dname, alpha):
    from oracle import oracle
    A, B, _ = _inputs(struct, dname)
    ref = oracle.spgemm(A, B, alpha=alpha, keep_zeros=True, sort=True)
    for a in ref:
        a.setflags(write=False)
    return ref


def reference(case, alpha=1.0):
    """The oracle's C of a case, computed once and never written."""
    return _reference(CASE[case].struct, CASE[case].dname, alpha)


def alpha_of(dname):
    """The alpha != 1 of a case (complex for complex types)."""
    return (0.5 - 0.25j) if dname.startswith("c") else -0.75


def _bits(x):
    x = np.ascontiguousarray(x)
    rd = x.real.dtype
    return x.view(rd).view(np.uint32 if rd == np.float32 else np.uint64)


def assert_same(got, ref, what=""):
    """Row pointer, column indices and value bits equal: no tolerance, no NaN relaxation."""
    p, j, x = got[:3]
    rp, rj, rx = ref[:3]
    assert np.array_equal(np.asarray(p, dtype=np.int64), np.asarray(rp, dtype=np.int64)), f"{what}: row pointer"
    assert np.array_equal(j, rj), f"{what}: column indices differ at {np.flatnonzero(j != rj)[:5]}"
    assert x.dtype == rx.dtype, f"{what}: dtype {x.dtype} != {rx.dtype}"
    bad = np.flatnonzero(_bits(x) != _bits(rx))
    assert bad.size == 0, f"{what}: {bad.size} value components differ, first at {bad[:5]}"


# ---------------------------------------------------------------------------------------------
# The C ABI through ctypes (GPU only): the test chooses C's row-pointer type, not nnz(C).

@contextlib.contextmanager
def environ(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


class Uploaded:
    """A CSR matrix on the device with its row pointer in both widths (uploaded once per case)."""

    def __init__(self, M, device="cuda:0"):
        import torch
        self.shape, self.nnz, self.dtype = M.shape, M.nnz, M.dtype
        host = {"indptr32": M.indptr.astype(np.int32), "indptr64": M.indptr.astype(np.int64),
                "indices": M.indices.astype(np.int32), "values": np.array(M.data)}
        up = {k: torch.from_numpy(v).to(device) for k, v in host.items()}
        self.indptr = {32: up["indptr32"], 64: up["indptr64"]}
        self.indices, self.data = up["indices"], up["values"]
        self.device = device
        # a second upload of the same host arrays, never handed to the library
        self._arrays = up
        self._uploaded = {k: torch.from_numpy(v).to(device) for k, v in host.items()}

    def check_unchanged(self, what=""):
        """The device arrays handed to the library (row pointer in both widths, indices, values)
        are byte for byte what was uploaded."""
        import torch
        names = list(self._arrays)
        same = torch.stack([(self._arrays[k].view(torch.uint8) == self._uploaded[k].view(torch.uint8)).all()
                            for k in names]).cpu()       # (one synchronise for the four arrays)
        bad = [k for k, ok in zip(names, same.tolist()) if not ok]
        assert not bad, f"{what}: input arrays {bad} were written"

    def view(self, ip):
        from spmm_amd._lib import SpgCsr
        vt = {v: VALUE_TYPE[d] for d, v in DTYPES.items()}[self.dtype.type]
        return SpgCsr(self.shape[0], self.shape[1], self.nnz, self.indptr[ip].data_ptr(), self.indices.data_ptr(),
                      self.data.data_ptr(), ip, vt)


def _scalar(dtype, v):
    """One host value of a value type for the C ABI (a (re, im) pair if complex)."""
    ct = ctypes.c_float if np.dtype(dtype).type in (np.float32, np.complex64) else ctypes.c_double
    if np.dtype(dtype).kind == "c":
        return (ct * 2)(complex(v).real, complex(v).imag)
    return ct(float(v))


def _in_workspace(ws, ptr, nbytes, dtype, what):
    """The `nbytes` at device address `ptr` as a tensor: a view of the guarded workspace `ws`,
    which must hold all of them inside its interior."""
    off = ptr - ws.data_ptr()
    assert 0 <= off and off + nbytes <= ws.nbytes, f"{what}: [{off}, {off + nbytes}) outside the {ws.nbytes}-byte workspace"
    return ws.bytes()[off:off + nbytes].view(dtype)


def run_abi(A, B, alg, alpha=1.0, cf=CF, ip=32, cp=32, env=None, info=None, fill=0xFF, ws=None, first_cp=None,
            in_place=False, extra=None):
    """C = alpha * A.B through spg_plan -> spg_symbolic -> spg_numeric with row pointers of `ip`
    bits for A and B and `cp` bits for C.  A, B: scipy CSR matrices or Uploaded.  alg 1, 2, 3 or
    "3c" (ALG3 with its chunks kept: SPG_ALG3_CHUNK_ALWAYS).  Returns (indptr, indices, data) as
    numpy arrays, indptr in the width asked for; `info` (a dict) receives the plan's plan_info.

    The workspace (exactly the queried size), C's row pointer, C's indices and C's values are
    guarded buffers (tests/guarded.py) poisoned with the byte `fill`: an entry the kernels leave
    unwritten keeps the poison, and all four guards are checked after the final synchronize, as
    are A's and B's device arrays against what was uploaded.
      ws: a guarded workspace to run in as it stands (at least the queried size; never refilled
        here) instead of a fresh one.
      first_cp: call spg_symbolic with a guarded row pointer of that width first, then again with
        `cp` (the header's repeated call); extra["first"] = (that row pointer, its nnzC).
      in_place: C's indices and values are the workspace views spg_result_in_workspace names
        (which must exist): spg_numeric only scales.
      extra (a dict) also receives "in_workspace" (spg_result_in_workspace returned pointers),
        "nnz" and "workspace_bytes"."""
    import torch
    from spmm_amd import _lib
    from tests.guarded import guarded
    dA = A if isinstance(A, Uploaded) else Uploaded(A)
    dB = B if isinstance(B, Uploaded) else Uploaded(B)
    dev = dA.device
    h = _lib.get_handle(torch.device(dev).index or 0)
    h.set_stream(torch.cuda.current_stream().cuda_stream)
    lib = h.lib
    env = dict(env or {})
    if alg == "3c":
        env["SPG_ALG3_CHUNK_ALWAYS"] = "1"
    algo = 3 if alg == "3c" else int(alg)
    va, vb = dA.view(ip), dB.view(ip)
    m, n = dA.shape[0], dB.shape[1]
    cplx = np.dtype(dA.dtype).kind == "c"
    ct = ctypes.c_float if dA.dtype.type in (np.float32, np.complex64) else ctypes.c_double
    al = (ct * 2)(complex(alpha).real, complex(alpha).imag) if cplx else ct(float(alpha))
    tdt = {np.float32: torch.float32, np.float64: torch.float64, np.complex64: torch.complex64,
           np.complex128: torch.complex128}[dA.dtype.type]
    what = f"alg={alg} IP={ip} CP={cp} fill={fill:#04x}"
    extra = {} if extra is None else extra
    with environ(env):
        wsb = ctypes.c_size_t(0)
        _lib.check(lib.spg_plan(h.ptr, ctypes.byref(va), ctypes.byref(vb), algo, cf, ctypes.byref(wsb), None, None),
                   "spg_plan")
        if ws is None:      # the queried size, not a byte more
            ws = guarded(wsb.value, "uint8", fill, dev, "workspace")
        assert ws.nbytes >= wsb.value, (ws.nbytes, wsb.value)
        extra["workspace_bytes"] = wsb.value
        plan = ctypes.c_void_p()
        _lib.check(lib.spg_plan(h.ptr, ctypes.byref(va), ctypes.byref(vb), algo, cf, ctypes.byref(wsb),
                                ctypes.c_void_p(ws.data_ptr()), ctypes.byref(plan)), "spg_plan")
        try:
            if info is not None:
                pi = _lib.SpgPlanInfo()
                _lib.check(lib.spg_plan_info(plan, ctypes.byref(pi), None, 0), "spg_plan_info")
                rows = (ctypes.c_int64 * (pi.n_chunks + 1))()
                _lib.check(lib.spg_plan_info(plan, ctypes.byref(pi), rows, pi.n_chunks + 1), "spg_plan_info")
                info.update({"path": ("general", "short", "tile")[pi.path], "tile_width": pi.tile_width,
                             "tiles_per_row": pi.tiles_per_row, "dense_tiles": bool(pi.dense_tiles),
                             "lds_ordered": bool(pi.lds_ordered), "record_group": int(pi.record_group),
                             "chunk_rows": [int(x) for x in rows]})
            nnz = ctypes.c_int64(0)
            first = None
            if first_cp is not None:
                first = guarded(m + 1, f"int{first_cp}", fill, dev, "C.indptr (first spg_symbolic)")
                _lib.check(lib.spg_symbolic(h.ptr, plan, ctypes.c_void_p(first.data_ptr()), first_cp,
                                            ctypes.byref(nnz)), "spg_symbolic")
                first_nnz = int(nnz.value)
                nnz = ctypes.c_int64(0)
            indptr = guarded(m + 1, f"int{cp}", fill, dev, "C.indptr")
            _lib.check(lib.spg_symbolic(h.ptr, plan, ctypes.c_void_p(indptr.data_ptr()), cp, ctypes.byref(nnz)),
                       "spg_symbolic")
            nz = int(nnz.value)
            pj, px = ctypes.c_void_p(), ctypes.c_void_p()
            _lib.check(lib.spg_result_in_workspace(plan, ctypes.byref(pj), ctypes.byref(px)), "spg_result_in_workspace")
            assert bool(pj.value) == bool(px.value)
            extra["in_workspace"], extra["nnz"] = bool(pj.value), nz
            gj = gx = None
            if in_place:
                assert pj.value and px.value, f"{what}: C is not in the workspace"
                cj = _in_workspace(ws, pj.value, 4 * nz, torch.int32, what + " C.indices")
                cx = _in_workspace(ws, px.value, np.dtype(dA.dtype).itemsize * nz, tdt, what + " C.values")
                jp, xp = pj.value, px.value
            else:
                gj = guarded(nz, "int32", fill, dev, "C.indices")
                gx = guarded(nz, dA.dtype, fill, dev, "C.values")
                cj, cx, jp, xp = gj.t, gx.t, gj.data_ptr(), gx.data_ptr()
            vc = _lib.SpgCsr(m, n, nz, indptr.data_ptr(), jp, xp, cp, va.value_type)
            _lib.check(lib.spg_numeric(h.ptr, plan, ctypes.byref(al), ctypes.byref(vc)), "spg_numeric")
            torch.cuda.synchronize()
        finally:
            lib.spg_plan_destroy(plan)
    out = indptr.t.cpu().numpy(), cj.cpu().numpy(), cx.cpu().numpy()
    for g in (ws, indptr, first, gj, gx):
        if g is not None:
            g.check(f"{what} {g.name}")
    dA.check_unchanged(what + " A")
    dB.check_unchanged(what + " B")
    if first is not None:
        extra["first"] = (first.t.cpu().numpy(), first_nnz)
    return out


def run_python(A, B, alg=2, alpha=1.0):
    """One product through cusparse.spgemm with int64 indptr tensors (the shim's itype branch)."""
    import torch
    from spmm_amd import cusparse
    from spmm_amd.sparse import csr_matrix
    dA, dB = csr_matrix(A.copy(), device="cuda:0"), csr_matrix(B.copy(), device="cuda:0")
    dA.indptr, dB.indptr = dA.indptr.to(torch.int64), dB.indptr.to(torch.int64)
    C = cusparse.spgemm(dA, dB, alpha=alpha, alg=alg)
    torch.cuda.synchronize()
    return C.indptr.cpu().numpy(), C.indices.cpu().numpy(), C.data.cpu().numpy()


def _handle_views(A, B, ip):
    import torch
    from spmm_amd import _lib
    dA = A if isinstance(A, Uploaded) else Uploaded(A)
    dB = B if isinstance(B, Uploaded) else Uploaded(B)
    h = _lib.get_handle(torch.device(dA.device).index or 0)
    h.set_stream(torch.cuda.current_stream().cuda_stream)
    return dA, dB, h, dA.view(ip), dB.view(ip)


def workspace_bytes(A, B, alg, cf=CF, ip=32, env=None):
    """spg_plan's size query."""
    from spmm_amd import _lib
    dA, dB, h, va, vb = _handle_views(A, B, ip)
    env = dict(env or {})
    if alg == "3c":
        env["SPG_ALG3_CHUNK_ALWAYS"] = "1"
    wsb = ctypes.c_size_t(0)
    with environ(env):
        _lib.check(h.lib.spg_plan(h.ptr, ctypes.byref(va), ctypes.byref(vb), 3 if alg == "3c" else int(alg), cf,
                                  ctypes.byref(wsb), None, None), "spg_plan")
    return int(wsb.value)


def run_ws(A, B, alg, alpha=1.0, cf=CF, ip=32, cp=32, env=None, fill=0xFF):
    """C = alpha * A.B through spg_spgemm_ws on a guarded workspace of the queried size and a
    guarded row pointer: C in the workspace (ALG1 single pass: views of it, which must lie inside
    it) or, with the live plan the call returns, spg_numeric into guarded arrays.  Returns
    (indptr, indices, data), in_workspace."""
    import torch
    from spmm_amd import _lib
    from tests.guarded import guarded
    dA, dB, h, va, vb = _handle_views(A, B, ip)
    lib, dev = h.lib, dA.device
    m, n = dA.shape[0], dB.shape[1]
    what = f"spg_spgemm_ws alg={alg} IP={ip} CP={cp} fill={fill:#04x}"
    al = _scalar(dA.dtype, alpha)
    tdt = guarded(0, dA.dtype).t.dtype
    with environ(dict(env or {})):
        ws = guarded(workspace_bytes(dA, dB, alg, cf, ip, env), "uint8", fill, dev, "workspace")
        indptr = guarded(m + 1, f"int{cp}", fill, dev, "C.indptr")
        nnz, peak = ctypes.c_int64(0), ctypes.c_size_t(0)
        pj, px, plan = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        _lib.check(lib.spg_spgemm_ws(h.ptr, ctypes.byref(va), ctypes.byref(vb), int(alg), cf, ctypes.byref(al),
                                     ctypes.c_void_p(ws.data_ptr()), ws.nbytes, ctypes.c_void_p(indptr.data_ptr()), cp,
                                     ctypes.byref(nnz), ctypes.byref(pj), ctypes.byref(px), ctypes.byref(peak),
                                     ctypes.byref(plan)), "spg_spgemm_ws")
        nz = int(nnz.value)
        gj = gx = None
        if plan.value:
            assert not pj.value and not px.value
            try:
                gj = guarded(nz, "int32", fill, dev, "C.indices")
                gx = guarded(nz, dA.dtype, fill, dev, "C.values")
                vc = _lib.SpgCsr(m, n, nz, indptr.data_ptr(), gj.data_ptr(), gx.data_ptr(), cp, va.value_type)
                _lib.check(lib.spg_numeric(h.ptr, plan, ctypes.byref(al), ctypes.byref(vc)), "spg_numeric")
                torch.cuda.synchronize()
            finally:
                lib.spg_plan_destroy(plan)
            cj, cx = gj.t, gx.t
        else:
            assert nz == 0 or (pj.value and px.value), what
            torch.cuda.synchronize()
            cj = (_in_workspace(ws, pj.value, 4 * nz, torch.int32, what + " C.indices") if nz
                  else torch.empty(0, dtype=torch.int32, device=dev))
            cx = (_in_workspace(ws, px.value, np.dtype(dA.dtype).itemsize * nz, tdt, what + " C.values") if nz
                  else torch.empty(0, dtype=tdt, device=dev))
    out = indptr.t.cpu().numpy(), cj.cpu().numpy(), cx.cpu().numpy()
    for g in (ws, indptr, gj, gx):
        if g is not None:
            g.check(f"{what} {g.name}")
    dA.check_unchanged(what + " A")
    dB.check_unchanged(what + " B")
    return out, not plan.value


def tile_groupings(tiles):
    """The value-tile ranges of every way spg_numeric_tiles is driven here: one range per tile,
    two groups, all tiles in one call -- each in ascending and in descending tile order."""
    if tiles == 1:       # (a single value tile: every grouping is the one call)
        return [("all/ascending", [(0, 1)])]
    per_tile = [(t, t + 1) for t in range(tiles)]
    two = [(0, tiles // 2), (tiles // 2, tiles)]
    return [("per-tile/ascending", per_tile), ("per-tile/descending", per_tile[::-1]), ("two/ascending", two),
            ("two/descending", two[::-1]), ("all/ascending", [(0, tiles)])]


def run_tiles(A, B, alpha=1.0, ip=32, cp=32, env=None, fill=0xFF):
    """The numeric phase by value tiles through the C ABI: one ALG2 plan, spg_tile_values into a
    guarded nnz(B) buffer, spg_symbolic, then for every grouping of tile_groupings() a fresh
    poisoned guarded C filled by spg_numeric_tiles calls.  Returns {grouping: (indptr, indices,
    data)}, {grouping: [poisoned entries of C left after each call]} and the value-tile count."""
    import torch
    from spmm_amd import _lib
    from tests.guarded import guarded
    assert fill == 0xFF      # the poison must be told from a result: index -1, NaN value
    real_t = torch.float32 if np.dtype(A.dtype) in (np.float32, np.complex64) else torch.float64
    dA, dB, h, va, vb = _handle_views(A, B, ip)
    lib, dev = h.lib, dA.device
    m, n = dA.shape[0], dB.shape[1]
    al = _scalar(dA.dtype, alpha)
    results, left = {}, {}
    with environ(dict(env or {})):
        ws = guarded(workspace_bytes(dA, dB, 2, CF, ip, env), "uint8", fill, dev, "workspace")
        wsb = ctypes.c_size_t(ws.nbytes)
        plan = ctypes.c_void_p()
        _lib.check(lib.spg_plan(h.ptr, ctypes.byref(va), ctypes.byref(vb), 2, CF, ctypes.byref(wsb),
                                ctypes.c_void_p(ws.data_ptr()), ctypes.byref(plan)), "spg_plan")
        try:
            pi = _lib.SpgPlanInfo()
            _lib.check(lib.spg_plan_info(plan, ctypes.byref(pi), None, 0), "spg_plan_info")
            assert pi.path == 2 and pi.n_chunks == 1, (pi.path, pi.n_chunks)
            tiles = -(-pi.tiles_per_row // pi.record_group)
            offs = (ctypes.c_int64 * (tiles + 1))()
            _lib.check(lib.spg_tile_value_offsets(h.ptr, plan, offs, tiles + 1), "spg_tile_value_offsets")
            assert offs[0] == 0 and offs[tiles] == dB.nnz, list(offs)
            tm = guarded(dB.nnz, dA.dtype, fill, dev, "tile-major values")
            _lib.check(lib.spg_tile_values(h.ptr, plan, ctypes.c_void_p(tm.data_ptr())), "spg_tile_values")
            indptr = guarded(m + 1, f"int{cp}", fill, dev, "C.indptr")
            nnz = ctypes.c_int64(0)
            _lib.check(lib.spg_symbolic(h.ptr, plan, ctypes.c_void_p(indptr.data_ptr()), cp, ctypes.byref(nnz)),
                       "spg_symbolic")
            nz = int(nnz.value)
            for name, ranges in tile_groupings(tiles):
                what = f"spg_numeric_tiles {name} IP={ip} CP={cp}"
                gj = guarded(nz, "int32", fill, dev, "C.indices")
                gx = guarded(nz, dA.dtype, fill, dev, "C.values")
                vc = _lib.SpgCsr(m, n, nz, indptr.data_ptr(), gj.data_ptr(), gx.data_ptr(), cp, va.value_type)
                left[name] = []
                for t0, t1 in ranges:
                    _lib.check(lib.spg_numeric_tiles(h.ptr, plan, ctypes.byref(al), ctypes.byref(vc),
                                                     ctypes.c_void_p(tm.data_ptr()), t0, t1), "spg_numeric_tiles")
                    torch.cuda.synchronize()
                    left[name].append(int(((gj.t == -1) | torch.isnan(gx.t.view(real_t).view(nz, -1)).any(1)).sum()))
                results[name] = indptr.t.cpu().numpy(), gj.t.cpu().numpy(), gx.t.cpu().numpy()
                for g in (ws, indptr, tm, gj, gx):
                    g.check(f"{what} {g.name}")
        finally:
            lib.spg_plan_destroy(plan)
    dA.check_unchanged("spg_numeric_tiles A")
    dB.check_unchanged("spg_numeric_tiles B")
    return results, left, tiles


# ---------------------------------------------------------------------------------------------
# Two inputs outside the case table: ALG1's single pass giving up (tests/test_gpu_parity.py and
# tests/test_gpu_poisoned_products.py share them).

@functools.lru_cache(maxsize=1)
def estimate_overflow_pair():
    """(A, B): A's entries select B's ten longest rows, so C outgrows the size ALG1's single pass
    estimates from the expected product count, and the product is redone two-phase."""
    rng = np.random.default_rng(43)
    B = sp.random(2000, 3000, density=0.001, format="lil", random_state=rng)
    for r in range(10):
        B[r, rng.choice(3000, 1500, replace=False)] = rng.standard_normal(1500)
    B = sp.csr_matrix(B)
    rows, cols = [], []
    for i in range(3000):
        for c in rng.choice(10, 5, replace=False):
            rows.append(i); cols.append(c)
    A = sp.csr_matrix((rng.standard_normal(len(rows)), (rows, cols)), shape=(3000, 2000))
    for M in (A, B):
        M.sum_duplicates(); M.sort_indices()
    return A, B


@functools.lru_cache(maxsize=1)
def long_row_pair():
    """(A, B): a short-row shape with one A row of 300 entries, more than the 64 the single pass
    takes: the pass hands over to the two-phase path."""
    rng = np.random.default_rng(41)
    A = sp.random(3000, 2000, density=0.004, format="lil", random_state=rng)
    A[1234, :300] = rng.standard_normal(300)
    A = sp.csr_matrix(A)
    B = sp.random(2000, 3000, density=0.004, format="csr", random_state=rng)
    A.sort_indices(); B.sort_indices()
    return A, B


def alg1_estimate(A, B):
    """The entries ALG1's single pass sizes its output for (spg_plan, restated)."""
    return int(min(1.15 * A.nnz * (B.nnz / B.shape[0]) + 4096.0, float(A.shape[0]) * float(B.shape[1])))


COLS16_WIDTHS = (65535, 65536, 65537, 140000)     # 1, 1, 2 and 3 blocks of 65536 columns
# rows cols16_matrix places by hand: label -> row
COLS16_ROWS = {"empty": 0, "last-block": 1, "first-block": 2, "edges": 3, "last-column": 4, "all-blocks": 5,
               "empty2": 6}


@functools.lru_cache(maxsize=None)
def cols16_matrix(cols):
    """Canonical CSR for spg_cols16_split / spg_cols16_join, rows on the 65536-column blocks: an
    empty row, a row only in the last block, one only in the first, one entry on each side of
    every block edge, the last column alone, a row through every block, 300 random rows of 0..29,
    then column 0 alone and a short row in the last block."""
    rng = np.random.default_rng(seed_of("cols16", cols))
    nb = (cols + 65535) // 65536
    last0 = (nb - 1) * 65536
    last = lambda m: np.sort(rng.choice(np.arange(last0, cols), min(m, cols - last0), replace=False))
    edges = sorted({c for b in range(nb) for c in (b * 65536, min(cols, (b + 1) * 65536) - 1)})
    rows = [[], last(40), np.arange(0, 50), edges, [cols - 1], np.sort(rng.choice(cols, 700, replace=False)), []]
    rows += [np.sort(rng.choice(cols, int(rng.integers(0, 30)), replace=False)) for _ in range(300)]
    rows += [[0], last(3)]
    lens = np.array([len(r) for r in rows])
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    indices = np.concatenate([np.asarray(r, dtype=np.int32) for r in rows]).astype(np.int32)
    M = sp.csr_matrix((np.ones(len(indices)), indices, indptr), shape=(len(rows), cols))
    for a in (M.data, M.indices, M.indptr):
        a.setflags(write=False)
    return M


def cols16_split_host(M):
    """include/spgemm.h's 16-bit column format restated: (block_starts, lo16).  block_starts is
    rows x (ceil(cols / 65536) - 1) uint32, per row the offset from the row's start of its first
    entry with column >= c * 65536 (the row's length if there is none), c = 1, 2, ...; lo16 the
    low 16 bits of every column."""
    rows, cols = M.shape
    nb1 = max(0, (cols + 65535) // 65536 - 1)
    starts = np.zeros((rows, nb1), dtype=np.uint32)
    for r in range(rows):
        rc = M.indices[M.indptr[r]:M.indptr[r + 1]]
        starts[r] = [np.searchsorted(rc, (b + 1) * 65536) for b in range(nb1)]
    return starts, (M.indices & 0xFFFF).astype(np.uint16)


def cols16_join_host(M, starts, lo16):
    """The columns back from the split: an entry's high half is the number of block starts at or
    below its offset in the row."""
    out = np.empty(M.nnz, dtype=np.int32)
    for r in range(M.shape[0]):
        a, b = M.indptr[r], M.indptr[r + 1]
        hi = (starts[r][None, :] <= np.arange(b - a)[:, None]).sum(axis=1) if starts.shape[1] else np.zeros(b - a, int)
        out[a:b] = (hi.astype(np.int64) << 16) | lo16[a:b]
    return out


POISON_FILLS = (0x00, 0xFF)
POISON_WIDTHS = ((32, 64), (64, 32))
STALE_ORDER = (1, 2, "3c", 2)
_NONE = np.zeros(0, dtype=np.int32)


def run_poisoned(case):
    """Every product of a case on poisoned, guarded buffers (tests/test_gpu_poisoned_products.py):
    {key: (indptr, indices, data)}.  Keys:
      "fill/<alg>/<fill>"    both poisons under every algorithm, (IP, CP) alternating between
                             (32, 64) and (64, 32) so that both widths see both poisons;
      "resym/<alg>"          spg_symbolic into an int32 row pointer, again into an int64 one, then
                             spg_numeric; "resym-first/<alg>" holds the first row pointer and, as
                             `indices`, the two nnzC;
      "stale/<i>/<alg>"      ALG1, ALG2, "3c", ALG2 in ONE workspace sized for the largest query,
                             poisoned once and never refilled; fresh plan and C arrays each;
      "handoff/copy", "handoff/inplace"   ALG1 with alpha != 1 into guarded C arrays and, where
                             spg_result_in_workspace names them, in the workspace views;
      "ws/1", "ws/2"         spg_spgemm_ws, alpha != 1; "flags" holds as `indices`
                             [handoff in workspace, ws/1 in workspace, ws/2 in workspace]."""
    from tests.guarded import guarded
    c = CASE[case]
    A, B, _ = inputs(case)
    dA, dB = Uploaded(A), Uploaded(B)
    al = alpha_of(c.dname)
    out = {}
    for ai, alg in enumerate(ALGS):
        for fi, fill in enumerate(POISON_FILLS):
            ip, cp = POISON_WIDTHS[(ai + fi) % 2]
            out[f"fill/{alg}/{fill:#04x}"] = run_abi(dA, dB, alg, 1.0, CF, ip, cp, c.env, fill=fill)
    for alg in ALGS:
        ex = {}
        out[f"resym/{alg}"] = run_abi(dA, dB, alg, 1.0, CF, 32, 64, c.env, first_cp=32, extra=ex)
        out[f"resym-first/{alg}"] = (ex["first"][0], np.array([ex["first"][1], ex["nnz"]], dtype=np.int64), _NONE)
    size = max(workspace_bytes(dA, dB, alg, CF, 32, c.env) for alg in ALGS)
    ws = guarded(size, "uint8", 0xFF, dA.device, "workspace (shared, never refilled)")
    for i, alg in enumerate(STALE_ORDER):
        out[f"stale/{i}/{alg}"] = run_abi(dA, dB, alg, 1.0, CF, 32, 32, c.env, ws=ws)
    ex = {}
    out["handoff/copy"] = run_abi(dA, dB, 1, al, CF, 64, 64, c.env, extra=ex)
    if ex["in_workspace"]:
        out["handoff/inplace"] = run_abi(dA, dB, 1, al, CF, 64, 64, c.env, in_place=True, fill=0x00)
    flags = [int(ex["in_workspace"])]
    for alg in (1, 2):
        out[f"ws/{alg}"], inws = run_ws(dA, dB, alg, al, CF, 32, 64 if alg == 1 else 32, c.env,
                                        fill=0xFF if alg == 1 else 0x00)
        flags.append(int(inws))
    out["flags"] = (_NONE, np.array(flags, dtype=np.int64), _NONE)
    return out


def run_cross(case):
    """Every product of a case: {key: (indptr, indices, data)} and {key: plan_info}.  Keys:
    (alg, ip, cp) for the alpha = 1 cross, "alpha" for alpha != 1 at (64, 64) under ALG2,
    "python" for the Python entry point with int64 row pointers."""
    c = CASE[case]
    A, B, _ = inputs(case)
    dA, dB = Uploaded(A), Uploaded(B)
    out, infos = {}, {}
    for alg in ALGS:
        for ip, cp in WIDTHS:
            infos[(alg, ip, cp)] = {}
            out[(alg, ip, cp)] = run_abi(dA, dB, alg, 1.0, CF, ip, cp, c.env, infos[(alg, ip, cp)])
    out["alpha"] = run_abi(dA, dB, 2, alpha_of(c.dname), CF, 64, 64, c.env)
    with environ(c.env):
        out["python"] = run_python(A, B)
    return out, infos


def child_main(case, path, mode="cross"):
    """run_cross (mode "cross") or run_poisoned (mode "poisoned") in a fresh process (a switch
    read once per process), results to an .npz."""
    import json
    out, infos = run_cross(case) if mode == "cross" else (run_poisoned(case), {})
    arrs = {}
    for key, (p, j, x) in out.items():
        s = key if isinstance(key, str) else "|".join(str(v) for v in key)
        arrs[s + "|p"], arrs[s + "|j"], arrs[s + "|x"] = p, j, x
    arrs["infos"] = np.frombuffer(json.dumps({"|".join(str(v) for v in k): v for k, v in infos.items()}).encode(),
                                  dtype=np.uint8)
    np.savez(path, **arrs)


def load_child(path):
    import json
    z = np.load(path)
    infos = json.loads(bytes(z["infos"]).decode())
    keys = {k.rsplit("|", 1)[0] for k in z.files if k != "infos"}

    def key_of(s):
        if "|" not in s:
            return s
        a, ip, cp = s.split("|")
        return (a if a == "3c" else int(a), int(ip), int(cp))
    out = {key_of(s): (z[s + "|p"], z[s + "|j"], z[s + "|x"]) for s in keys}
    return out, {key_of(s): v for s, v in infos.items()}
