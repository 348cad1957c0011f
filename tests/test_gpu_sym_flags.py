"""The flag-map symbolic kernel (k_tile_sym_flag) against the bitmap kernels and the oracle.

No plan selects the flag kernel (it measured slower); SPG_SYM_FLAGS=1 runs it
for every dense-tile plan.  Every case runs with SPG_SYM_FLAGS=1 and with SPG_SYM_FLAGS=0
(never; the bitmap kernels share its walk); the variable is read per plan, so both run in this process.  Each
asserts a tile-path plan with dense numeric tiles and compares ALG1, ALG2 and chunked ALG3
(SPG_ALG3_CHUNK_ALWAYS) bit for bit with the CPU oracle.

The shapes are the smallest that reach each seam of the kernel.  The planner picks the numeric
tile from x = avgA * avgB / B.cols: fp64 tiles are dense (2048 columns) for 0.28 < x < 0.64 and
for x > 0.70, fp32 / complex tiles (1024 columns) for x > 0.65; each builder says where it sits.
"""
import os

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import oracle

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _values(rng, n, dtype):
    v = rng.standard_normal(n)
    if np.dtype(dtype).kind == "c":
        v = v + 1j * rng.standard_normal(n)
    return v.astype(dtype)


def _rows_exact(rng, lens, cols, dtype=np.float64, lo=0):
    """Canonical CSR whose row i holds exactly lens[i] distinct columns of [lo, lo + cols)
    (numpy, as test_gpu_parity._random_rows: no N^2 sampling); the shape is set by the caller."""
    idx = []
    for n in lens:
        n = int(n)
        cand = np.unique(rng.integers(0, cols, size=2 * n + 8))
        if cand.size < n:
            cand = np.arange(cols)
        idx.append(lo + np.sort(rng.choice(cand, size=n, replace=False)))
    indices = np.concatenate(idx).astype(np.int32) if idx else np.zeros(0, np.int32)
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return indptr, indices, _values(rng, indices.size, dtype)


def _csr(parts, shape):
    indptr, indices, data = parts
    M = sp.csr_matrix((data, indices, indptr), shape=shape)
    M.has_canonical_format = True
    return M


def _a_rows(rng, rows, k, lo, hi, dtype=np.float64, fixed=()):
    """A: `rows` rows of lo..hi entries over k columns; `fixed` = (row, entries) pairs."""
    lens = rng.integers(lo, hi + 1, size=rows)
    for r, n in fixed:
        lens[r] = n
    return _csr(_rows_exact(rng, lens, k, dtype), (rows, k))


def _exact_fit():
    """B 4096 x 65536: the flag map is exactly 64 KB (one whole-row symbolic tile, 32 numeric
    tiles).  B rows of 0, 1, 127, 128, 129, 385 and 900 entries (segments that end one column
    short of, at and one past a 128-column step, past the three prefetched steps, and seven
    steps long); A: 96 rows of 1 to 39 entries, most of them long so that x = 0.32, one empty,
    one of exactly 16 entries (one round: waves 1.. get none) and one of 17 (a second round of one
    entry)."""
    rng = np.random.default_rng(101)
    k, n = 4096, 65536
    blen = rng.choice([0, 1, 127, 128, 129, 385, 900], size=k, p=[0.03, 0.03, 0.04, 0.05, 0.05, 0.25, 0.55])
    B = _csr(_rows_exact(rng, blen, n), (k, n))
    alen = np.where(rng.random(96) < 0.85, rng.integers(36, 40, size=96), rng.integers(1, 36, size=96))
    alen[[3, 11, 12, 13, 14]] = [0, 16, 17, 1, 39]
    A = _csr(_rows_exact(rng, alen, k), (96, k))
    return A, B


def _ragged(ncols, dtype=np.float64):
    def build():
        rng = np.random.default_rng(102 + ncols)
        k = 1024
        if ncols == 2049:
            # x = 0.35: two 2048-column numeric tiles, the second one column wide (4096-byte map)
            blen = rng.choice([0, 1, 20, 36, 70], size=k, p=[0.05, 0.05, 0.3, 0.3, 0.3])
        else:
            # x = 0.95: 20000 columns pad to a 32768-byte map, the last numeric tile is partial
            blen = rng.choice([0, 1, 400, 900, 1700], size=k, p=[0.05, 0.05, 0.2, 0.4, 0.3])
        B = _csr(_rows_exact(rng, blen, ncols, dtype), (k, ncols))
        A = _a_rows(rng, 96, k, 1, 39, dtype, fixed=[(5, 0), (6, 16), (7, 17)])
        return A, B
    return build


def _several_symbolic_tiles():
    """B 1024 x 70000: two 65536-column symbolic tiles per row (per-entry tile bounds from the
    segment index, the second tile 4464 columns wide: 3 numeric tiles, the last partial).
    A rows of 60 to 140 entries and B rows of ~700 make x = 1.0, so the tiles are dense."""
    rng = np.random.default_rng(103)
    k, n = 1024, 70000
    blen = rng.choice([0, 300, 700, 1200], size=k, p=[0.05, 0.25, 0.4, 0.3])
    B = _csr(_rows_exact(rng, blen, n), (k, n))
    A = _a_rows(rng, 48, k, 60, 140, fixed=[(2, 0), (3, 16), (4, 17)])
    return A, B


def _collisions_same_sets():
    """Every B row holds the same 1200 columns: every store after a column's first hits a flag
    that is already set, from several waves at once (x = 0.37)."""
    rng = np.random.default_rng(104)
    k, n, m = 512, 65536, 1200
    cols = np.sort(rng.choice(n, size=m, replace=False)).astype(np.int32)
    B = _csr((np.arange(k + 1, dtype=np.int64) * m, np.tile(cols, k), _values(rng, k * m, np.float64)), (k, n))
    A = _a_rows(rng, 64, k, 1, 39, fixed=[(0, 39), (1, 16)])
    return A, B


def _collisions_one_tile():
    """Every B column lies in numeric tile 5 of 32 (1500 of its 2048 columns per B row): 31 tiles
    count zero (x = 0.46)."""
    rng = np.random.default_rng(105)
    k, n = 512, 65536
    B = _csr(_rows_exact(rng, np.full(k, 1500), 2048, lo=5 * 2048), (k, n))
    A = _a_rows(rng, 64, k, 1, 39, fixed=[(0, 39), (1, 16)])
    return A, B


CASES = {
    "exact_fit_64k": _exact_fit,
    "ragged_20000": _ragged(20000),
    "ragged_2049": _ragged(2049),
    "two_symbolic_tiles_70000": _several_symbolic_tiles,
    "collisions_same_sets": _collisions_same_sets,
    "collisions_one_tile": _collisions_one_tile,
    "ragged_20000_fp32": _ragged(20000, np.float32),
    "ragged_20000_complex128": _ragged(20000, np.complex128),
}


def _bits(x):
    return np.ascontiguousarray(x).view({4: np.uint32, 8: np.uint64, 16: np.uint64}[x.dtype.itemsize])


def _product(dA, dB, alg):
    from spmm_amd import cusparse
    if alg == "3c":
        os.environ["SPG_ALG3_CHUNK_ALWAYS"] = "1"
    try:
        C = cusparse.spgemm(dA, dB, alg=3 if alg == "3c" else alg, chunk_fraction=0.1 if alg == "3c" else 0.2)
        torch.cuda.synchronize()
    finally:
        os.environ.pop("SPG_ALG3_CHUNK_ALWAYS", None)
    return C.indptr.cpu().numpy().astype(np.int64), C.indices.cpu().numpy(), C.data.cpu().numpy()


@pytest.mark.parametrize("name", list(CASES))
def test_flag_kernel_bitexact(name, monkeypatch):
    from spmm_amd import cusparse
    from spmm_amd.sparse import csr_matrix
    A, B = CASES[name]()
    rp, rj, rx = oracle.spgemm(A, B, keep_zeros=True, sort=True)
    dA, dB = csr_matrix(A, device=DEV), csr_matrix(B, device=DEV)
    for flags in ("1", "0"):
        monkeypatch.setenv("SPG_SYM_FLAGS", flags)
        info = cusparse.plan_info(dA, dB, alg=2)
        assert info["path"] == "tile", info
        assert info["dense_tiles"], info
        for alg in (1, 2, "3c"):
            p, j, x = _product(dA, dB, alg)
            what = f"SPG_SYM_FLAGS={flags} alg {alg}"
            assert np.array_equal(p, rp), f"{what}: row pointer"
            assert np.array_equal(j, rj), f"{what}: column indices"
            assert x.dtype == rx.dtype
            assert np.array_equal(_bits(x), _bits(rx)), f"{what}: values"
