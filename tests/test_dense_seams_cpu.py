"""tests/dense_seams.py is not vacuous: every group of seam_matrix has the entry total its table
says, the straddling and long rows cross the chunk boundaries they are meant to cross, the
row-count and row-major matrices hold the lengths their tests rely on, and the references used on
the GPU (oracle.spmv / oracle.spmm) equal scipy's products bit for bit on exactly these inputs."""
import numpy as np
import pytest

from oracle import oracle
from tests import dense_seams as ds
from tests import special_values as sv
from tests.instantiations import DTYPES, alpha_of

CHS = [ds.SPMV_CH, ds.SPMM_CH]


def _bits(v):
    return np.ascontiguousarray(v).view(np.uint8)


def _group(A, name):
    r0 = ds.group_start(name)
    r1 = min(A.shape[0], r0 + ds.WAVE)
    p = A.indptr.astype(np.int64)
    return r0, r1, p, p[r0:r1 + 1] - p[r0]          # offsets relative to the group's first entry


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("ch", CHS)
def test_seam_matrix_groups(ch, dname):
    A = ds.seam_matrix(ch, dname)
    assert A.shape == (728, 4096) == (ds.ROWS, ds.COLS) and A.dtype == DTYPES[dname]
    assert A.has_canonical_format and A.indptr.dtype == np.int32
    assert ds.seam_matrix(ch, DTYPES[dname]) is A
    L = 2 * ch + 452
    total = {}
    for g in ds.GROUPS:
        r0, r1, p, off = _group(A, g)
        assert r1 - r0 == (24 if g == "ragged" else 64), g
        total[g] = int(off[-1])
    assert total["empty"] == 0
    assert total["one"] == 1 and np.diff(_group(A, "one")[3])[-1] == 1
    assert total["ch-1"] == ch - 1 and total["ch"] == ch
    for g in ("ch-1", "ch"):
        lens = np.diff(_group(A, g)[3])
        assert lens.max() - lens.min() <= 1, g
    # ch+1: the 63 first rows fill the first chunk exactly, the last row's entry is alone in the second
    off = _group(A, "ch+1")[3]
    assert total["ch+1"] == ch + 1 and off[63] == ch and off[64] - off[63] == 1
    # 2ch: the empty row 31 sits exactly on the chunk boundary
    r0, _, p, off = _group(A, "2ch")
    assert total["2ch"] == 2 * ch
    assert p[r0 + 31] == p[r0 + 32] == p[r0] + ch
    assert (np.diff(off)[:31] > 0).all() and (np.diff(off)[32:] > 0).all()
    # straddle: row 10's first and last entry lie in different chunks
    off = _group(A, "straddle")[3]
    assert total["straddle"] == 2 * ch + 1
    assert off[10] == ch - 32 and off[11] - off[10] == 65
    assert off[10] // ch == 0 and (off[11] - 1) // ch == 1
    # the long rows: L entries over three chunks or more, at lanes 0, 63 and 31 (between two empty rows)
    for g, lane in ds.LONG_LANE.items():
        off = _group(A, g)[3]
        lens = np.diff(off)
        assert lens[lane] == L and (np.delete(lens, lane) <= 8).all(), g
        assert (off[lane + 1] - 1) // ch - off[lane] // ch + 1 >= 3, g
        assert total[g] == L + int(np.delete(lens, lane).sum())
    lens = np.diff(_group(A, "long-mid")[3])
    assert lens[30] == 0 and lens[32] == 0
    lens = np.diff(_group(A, "random")[3])
    assert 30 <= lens.max() <= 40 and lens.min() <= 5 and total["random"] > 512
    lens = np.diff(_group(A, "ragged")[3])
    assert len(lens) == 24 and lens[-1] == 130 and lens[:-1].max() <= 40
    assert A.nnz == sum(total.values())
    # the fixed totals (7 * ch + 2), three long rows (6 * ch + 1356) and about 2100 random entries:
    # about 17 000 entries at ch = 1024, about 10 700 at ch = 512
    assert abs(A.nnz - {1024: 17000, 512: 10700}[ch]) < 600, A.nnz
    # twelve waves fill three blocks of four; the ragged group is the last block's fourth wave
    assert -(-A.shape[0] // ds.WAVE) == 3 * ds.WPB and A.shape[0] % ds.WAVE == 24


@pytest.mark.parametrize("dname", list(DTYPES))
def test_row_count_and_row_major_matrices(dname):
    for rows in ds.ROW_COUNTS:
        A = ds.row_count_matrix(rows, dname)
        lens = np.diff(A.indptr)
        assert A.shape == (rows, 257) and A.has_canonical_format and lens.max() <= 12
        if rows >= 63:
            assert lens.min() == 0 and lens.max() == 12, rows
    assert ds.ROW_COUNTS == [1, 63, 64, 65, 255, 256, 257]
    A = ds.row_major_matrix(dname)
    lens = np.diff(A.indptr)
    assert A.shape == (71, 256) and A.has_canonical_format
    assert set(lens) == set(ds.ROW_MAJOR_LENGTHS) == {0, 1, 3, 4, 5, 7, 8, 9, 63, 64, 65, 71, 72, 73, 127, 128, 129,
                                                       200}
    assert list(lens[:18]) == ds.ROW_MAJOR_LENGTHS and list(lens[54:]) == ds.ROW_MAJOR_LENGTHS[:17]


@pytest.mark.parametrize("dname", list(DTYPES))
def test_oracle_equals_scipy_on_these_inputs(dname):
    dt = DTYPES[dname]
    mats = [ds.seam_matrix(ch, dname) for ch in CHS] + [ds.row_count_matrix(r, dname) for r in ds.ROW_COUNTS]
    mats.append(ds.row_major_matrix(dname))
    for A in mats:
        x = ds.dense_values("x", (A.shape[1],), dt)
        got = oracle.spmv(A, x)
        assert got.dtype == dt and np.array_equal(_bits(got), _bits(A @ x))
        for n in (1, 9):
            X = ds.dense_values("B", (A.shape[1], n), dt)
            got = oracle.spmm(A, X)
            assert got.dtype == dt and np.array_equal(_bits(got), _bits(A @ X))
        # an empty row's sum is +0 and stays a zero under alpha
        empty = np.flatnonzero(np.diff(A.indptr) == 0)
        y = oracle.spmv(A, x)
        assert (y[empty] == 0).all() and not np.signbit(y[empty].real).any()


def test_epilogue_restatement():
    """special_values.axpby, the reference of the GPU epilogue: alpha == 1 and beta == 0 take
    their shortcuts, the complex product is spelled out on the parts."""
    for dname, dt in DTYPES.items():
        s = ds.dense_values("s", (50,), dt)
        y = ds.dense_values("y", (50,), dt)
        al, be = alpha_of(dname), ds.beta_of(dname)
        assert sv.axpby(1.0, s, 0.0, y) is s
        v = sv.axpby(al, s, be, y)
        assert v.dtype == dt
        np.testing.assert_allclose(v, dt(al) * s + dt(be) * y, rtol=1e-5 if dt in (np.float32, np.complex64) else 1e-14)
        nan = np.full(50, np.nan, dtype=dt)
        assert np.array_equal(_bits(sv.axpby(al, s, 0.0, nan)), _bits(sv.cmul(al, s)))
