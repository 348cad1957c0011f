"""The canonicalisation rule without a GPU: tests/canon_cases.py's numpy restatement against scipy
wherever scipy is determinate, and the containers' torch paths (CPU tensors) against the
restatement -- csr_matrix.sum_duplicates / eliminate_zeros, coo_matrix.tocsr and coo_matrix's
in-place sum_duplicates / eliminate_zeros."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import canon_cases as cc          # noqa: E402
from tests import special_values as sv       # noqa: E402

DT = list(cc.DTYPES.items())
IDS = [k for k, _ in DT]


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint8)


# ------------------------------------------------------------------ the restatement against scipy
@pytest.mark.parametrize("name,dt", DT, ids=IDS)
def test_sum_structure_always_equals_scipy(name, dt):
    m, n = 40, 300
    rows, cols, vals = cc.pool_triplets(m, n, 6000, 2500, dt, seed=11)
    p, j, x = cc.as_csr(m, rows, cols, vals)
    assert np.diff(p).max() > 16                       # long rows: scipy's order of addition is open here
    S = cc.scipy_csr((m, n), p, j, x)
    S.sum_duplicates()
    rp, rj, rx = cc.restate((m, n), cc.rows_of(p), j, x, cc.SUM)
    assert np.array_equal(rp, S.indptr) and np.array_equal(rj, S.indices)
    assert rj.size < j.size


@pytest.mark.parametrize("kind", ["short_rows", "mult2"])
@pytest.mark.parametrize("name,dt", DT, ids=IDS)
def test_sum_values_equal_scipy_where_it_is_determinate(name, dt, kind):
    m, n = 300, 500
    if kind == "short_rows":
        rows, cols, vals = cc.short_row_triplets(m, n, dt, seed=21)
    else:
        rows, cols, vals = cc.mult2_triplets(m, n, 9000, 0.4, dt, seed=22)
    p, j, x = cc.as_csr(m, rows, cols, vals)
    if kind == "short_rows":
        assert np.diff(p).max() <= 16
    S = cc.scipy_csr((m, n), p, j, x)
    S.sum_duplicates()
    ref = cc.restate((m, n), cc.rows_of(p), j, x, cc.SUM)
    assert ref[1].size < j.size                        # duplicates were there
    sv.assert_same_special(ref, (S.indptr, S.indices, S.data))
    assert np.array_equal(_bits(ref[2]), _bits(S.data))
    # the COO form of the same triplets gives the same matrix
    coo = cc.restate((m, n), rows, cols, vals, cc.SUM, coo=True)
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(coo, ref))


@pytest.mark.parametrize("name,dt", DT, ids=IDS)
def test_drop_zeros_alone_equals_scipy_array_for_array(name, dt):
    m, n = 50, 70
    rows, cols, vals = cc.pool_triplets(m, n, 3000, 1500, dt, seed=31)
    vals[::7] = 0
    vals[3::11] = -vals[3::11] * 0                      # -0.0 / (+-0, +-0)
    p, j, x = cc.as_csr(m, rows, cols, vals)
    S = cc.scipy_csr((m, n), p, j, x)
    S.eliminate_zeros()
    ref = cc.restate((m, n), cc.rows_of(p), j, x, cc.DROP)
    assert ref[1].size < j.size
    assert np.array_equal(ref[0], S.indptr) and np.array_equal(ref[1], S.indices)
    assert np.array_equal(_bits(ref[2]), _bits(S.data))


@pytest.mark.parametrize("name,dt", DT, ids=IDS)
def test_sort_without_duplicates_equals_sort_indices(name, dt):
    m, n = 60, 4000
    rows, cols, vals = cc.distinct_triplets(m, n, 5000, dt, seed=41)
    p, j, x = cc.as_csr(m, rows, cols, vals)
    S = cc.scipy_csr((m, n), p, j, x)
    S.sort_indices()
    ref = cc.restate((m, n), cc.rows_of(p), j, x, cc.SORT)
    assert not np.array_equal(ref[1], j)
    assert np.array_equal(ref[0], S.indptr) and np.array_equal(ref[1], S.indices)
    assert np.array_equal(_bits(ref[2]), _bits(S.data))


def test_coo_with_no_op_is_coo_tocsr():
    import scipy.sparse as sp
    m, n = 30, 40
    rows, cols, vals = cc.pool_triplets(m, n, 2000, 600, np.float64, seed=51)
    p, j, x = cc.restate((m, n), rows, cols, vals, 0, coo=True)
    M = sp.coo_matrix((vals, (rows, cols)), shape=(m, n))
    ip, ij, ix = np.zeros(m + 1, np.int32), np.zeros(vals.size, np.int32), np.zeros(vals.size)
    sp._sparsetools.coo_tocsr(m, n, vals.size, M.row.astype(np.int32), M.col.astype(np.int32), M.data, ip, ij, ix)
    assert np.array_equal(p, ip) and np.array_equal(j, ij) and np.array_equal(_bits(x), _bits(ix))


def test_stored_order_decides_the_sum():
    a, b = cc.order_pair(np.float64)
    ra, rb = (cc.restate(a[0], *a[1:], cc.SUM, coo=True) for a in (a, b))
    assert np.array_equal(ra[1], rb[1]) and not np.array_equal(_bits(ra[2]), _bits(rb[2]))


# ------------------------------------------------------------------ the torch paths (CPU tensors)
def _csr_cpu(shape, p, j, x):
    from spmm_amd.sparse import csr_matrix
    return csr_matrix((torch.from_numpy(x.copy()), torch.from_numpy(j.copy()), torch.from_numpy(p.copy())),
                      shape=shape, device="cpu", canonical=False)


def _parts(M):
    return M.indptr.numpy(), M.indices.numpy(), M.data.numpy()


@pytest.mark.parametrize("name,dt", DT, ids=IDS)
def test_torch_sum_duplicates_matches_the_rule(name, dt):
    m, n = 40, 300
    rows, cols, vals = cc.pool_triplets(m, n, 4000, 1500, dt, seed=61)
    p, j, x = cc.as_csr(m, rows, cols, vals)
    M = _csr_cpu((m, n), p, j, x)
    M.sum_duplicates()
    sv.assert_same_special(_parts(M), cc.restate((m, n), cc.rows_of(p), j, x, cc.SUM))
    assert M.has_canonical_format


@pytest.mark.parametrize("name,dt", DT, ids=IDS)
def test_torch_eliminate_zeros_matches_the_rule(name, dt):
    m, n = 40, 300
    rows, cols, vals = cc.pool_triplets(m, n, 4000, 1500, dt, seed=62)
    vals[::5] = 0
    p, j, x = cc.as_csr(m, rows, cols, vals)
    M = _csr_cpu((m, n), p, j, x)
    M.eliminate_zeros()
    sv.assert_same_special(_parts(M), cc.restate((m, n), cc.rows_of(p), j, x, cc.DROP))


@pytest.mark.parametrize("name,dt", DT, ids=IDS)
def test_torch_coo_paths_match_the_rule(name, dt):
    from spmm_amd.sparse import coo_matrix
    m, n = 40, 300
    rows, cols, vals = cc.pool_triplets(m, n, 4000, 1500, dt, seed=63)
    vals[::5] = 0

    def coo():
        return coo_matrix((torch.from_numpy(vals.copy()), (torch.from_numpy(rows.copy()), torch.from_numpy(cols.copy()))),
                          shape=(m, n), device="cpu")
    ref = cc.restate((m, n), rows, cols, vals, cc.SUM, coo=True)
    sv.assert_same_special(_parts(coo().tocsr()), ref)
    # in place, the matrix stays COO: the entries of the CSR result with their rows spelled out
    C = coo()
    C.sum_duplicates()
    assert C.format == "coo" and C.row.dtype == torch.int64 and C.col.dtype == torch.int64
    assert np.array_equal(C.row.numpy(), cc.rows_of(ref[0])) and np.array_equal(C.col.numpy(), ref[1])
    sv.assert_values_special(C.data.numpy(), ref[2])
    # eliminate_zeros keeps the stored order
    Z = coo()
    Z.eliminate_zeros()
    keep = vals != 0
    assert 0 < keep.sum() < vals.size
    assert np.array_equal(Z.row.numpy(), rows[keep]) and np.array_equal(Z.col.numpy(), cols[keep])
    assert np.array_equal(_bits(Z.data.numpy()), _bits(vals[keep]))
