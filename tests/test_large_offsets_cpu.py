"""tests/large_offsets.py against scipy and the oracle at scaled-down geometries, on CPU tensors:
the builder and every expected-result model that tests/test_gpu_large_offsets.py holds the kernels
to, compared on the whole matrix, array for array and bit for bit.  The reference matrix is built
from the definition (a Python loop over rows and columns), not from the builder's closed forms.
The full-size geometry's arithmetic is asserted without allocating it.  This is what makes a
failure on the device the kernel's fault and not the model's.
"""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import oracle
from tests import canon_cases as cc
from tests import large_offsets as lo
from tests import special_values as sv

torch = pytest.importorskip("torch")

# (pad_rows, L, W, entries per slice, the offset that stands in for 2**31)
SMALL = {
    "1000x250": (1000, 250, 256, 1 << 14, 125077),      # 16 slices; offset 125077 lies inside row 500
    "517x250": (517, 250, 256, 1 << 15, 250 * 300),     # pad_rows no multiple of W; no row straddles
    "1xW": (1, 256, 256, 1 << 14, 100),                 # one full row: L == W, no gap
    "300x3of8": (300, 3, 8, 64, 451),                   # a gap that wraps in most rows
}
NAMES = list(SMALL)


@functools.lru_cache(maxsize=None)
def geom(name):
    pad_rows, L, W, se, _ = SMALL[name]
    return lo.Geometry(pad_rows, L, W, slice_entries=se)


def boundary(name):
    return SMALL[name][4]


def _bits(v):
    return np.ascontiguousarray(v).view(np.uint8)


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.dtype}{got.shape} vs {want.dtype}{want.shape}"
    assert np.array_equal(_bits(got), _bits(want)), what


@functools.lru_cache(maxsize=None)
def reference(name, reverse=False, zeros=False):
    """(indptr, indices, values) of the whole matrix from the definition."""
    g = geom(name)
    cols, vals = [], []
    for i in range(g.pad_rows):
        c = [c for c in range(g.W) if (c + i) % g.W >= g.W - g.L]
        v = []
        for cj in c:
            x = (31 * i + 17 * cj) % 61 - 30
            x = float(31 if x == 0 else x)
            if zeros and (7 * i + 3 * cj) % 11 == 0:
                x = 0.0
            if zeros and (7 * i + 3 * cj) % 11 == 1:
                x = -0.0
            v.append(x)
        if reverse:
            c, v = c[::-1], v[::-1]
        cols += c
        vals += v
    indptr = np.concatenate([np.arange(g.pad_rows, dtype=np.int64) * g.L, g.tail.indptr.astype(np.int64) + g.pad_nnz])
    return (indptr, np.concatenate([np.array(cols, np.int32), g.tail.indices]),
            np.concatenate([np.array(vals, np.float32), g.tail.data]))


def scipy_of(name):
    g = geom(name)
    p, j, x = reference(name)
    A = sp.csr_matrix((x, j, p), shape=(g.rows, g.W))
    assert A.has_canonical_format
    return A


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("variant", ["forward", "reverse", "zeros"])
def test_builder_equals_the_definition(name, variant):
    g = geom(name)
    kw = dict(reverse=variant == "reverse", zeros=variant == "zeros")
    M = g.build("cpu", **kw)
    p, j, x = reference(name, **kw)
    _same(M.indptr.numpy(), p, "indptr")
    _same(M.indices.numpy(), j, "indices")
    _same(M.values.numpy(), x, "values")
    assert g.first_pad_difference(M, **kw) is None
    assert M.nnz == g.nnz == p[-1]
    for i in g.marked_rows(boundary(name)):
        c, v = g.pad_row_host(i, reverse=kw["reverse"])
        if not kw["zeros"]:
            _same(v, x[p[i]:p[i + 1]], f"pad_row_host({i}) values")
        _same(c, j[p[i]:p[i + 1]], f"pad_row_host({i}) columns")


def test_first_pad_difference_names_slice_row_and_offset():
    g = geom("1000x250")
    M = g.build("cpu")
    M.values[250 * 700 + 3] = 5.5
    assert g.first_pad_difference(M) == f"slice {700 // g.slice_rows}: row 700, offset {250 * 700 + 3}"
    M = g.build("cpu")
    M.indices[250 * 64] += 1
    assert g.first_pad_difference(M) == "slice 1: row 64, offset 16000"


@pytest.mark.parametrize("name", NAMES)
def test_wide_variant(name):
    g = geom(name)
    M = g.build("cpu", mul=lo.WIDE_MUL, cols=lo.WIDE_COLS, values=False)
    _same(M.indices.numpy(), reference(name)[1] * np.int32(lo.WIDE_MUL), "indices")
    assert int(M.indices.max()) < lo.WIDE_COLS and M.values is None


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("coefs", [(1.0, 0.0), (2.0, 0.5)])
def test_spmv_and_spmm_models(name, coefs):
    g, A = geom(name), scipy_of(name)
    alpha, beta = coefs
    x = lo.x_vector(g.W)
    i = np.arange(g.rows)
    y0 = (2 * ((3 * i) % 9 - 4)).astype(np.float32)
    _same(g.tail_y0(), y0[g.pad_rows:], "tail_y0")
    for X, Y0 in ((x, y0), (lo.b_matrix(g.W, 5), np.repeat(y0[:, None], 5, axis=1))):
        S = A @ X                                                     # scipy, float32, in entry order
        _same(S, oracle.spmv(A, X) if X.ndim == 1 else oracle.spmm(A, X), "oracle vs scipy")
        want = sv.axpby(alpha, S, beta, Y0)
        got = torch.cat([g.expect_product_pad(a, b, torch.from_numpy(np.array(X)), alpha, beta)
                         for a, b in g.row_slices()]).numpy()
        assert np.array_equal(got, want[:g.pad_rows]), "pad rows (numeric ==: the sign of a zero is not modelled)"
        assert not np.isnan(want).any()


@pytest.mark.parametrize("name", NAMES)
def test_transpose_model(name):
    g, A = geom(name), scipy_of(name)
    AT = A.tocsc()
    p = g.csc_indptr()
    _same(p, AT.indptr.astype(np.int64), "transpose row pointer")
    tp, tj, tx = g.csc_tail()
    _same(tx, g.tail.tocsc().data, "tail values")
    cnt = g.csc_pad_counts()
    if g.pad_rows % g.W == 0:
        assert (cnt == cnt[0]).all()
    for j in range(g.W):
        rows, vals = g.csc_pad_row(j, "cpu")
        n = int(cnt[j])
        _same(np.concatenate([rows.numpy(), tj[tp[j]:tp[j + 1]]]), AT.indices[p[j]:p[j + 1]], f"row {j} indices")
        _same(np.concatenate([vals.numpy(), tx[tp[j]:tp[j + 1]]]), AT.data[p[j]:p[j + 1]], f"row {j} values")
        assert rows.numel() == n


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("coefs", [(1, 1), (1, -1)])
def test_addition_model(name, coefs):
    g, A = geom(name), scipy_of(name)
    alpha, beta = coefs
    touched, Bs = g.small_operand(boundary=boundary(name))
    marked = g.marked_rows(boundary(name))
    assert list(touched[:len(marked)]) == marked and len(touched) == len(marked) + g.tail_rows
    s = g.straddling_row(boundary(name))
    assert s is None or s in marked
    # the small operand at full height, by scipy and by the builder
    Bd = g.spread_small(touched, Bs, "cpu")
    B = sp.csr_matrix((Bd.values.numpy(), Bd.indices.numpy(), Bd.indptr.numpy()), shape=A.shape)
    assert B.has_canonical_format and B.nnz == Bs.nnz
    assert (abs(B[touched] - Bs)).nnz == 0 and np.setdiff1d(np.flatnonzero(np.diff(B.indptr)), touched).size == 0
    for n, i in enumerate(marked):                 # every column the pad lacks in a marked row is in B
        gap = [c for c in range(g.W) if (c + i) % g.W < g.W - g.L]
        assert set(gap) <= set(Bs.indices[Bs.indptr[n]:Bs.indptr[n + 1]])
    C = (A + B) if beta == 1 else (A - B)
    C.sort_indices()
    assert np.count_nonzero(C.data) == C.nnz
    Cs, extra = g.expect_sum(touched, Bs, alpha, beta)
    assert extra[-1] == C.nnz - A.nnz
    _same(g.touched_rows_of_A(touched).toarray(), A[touched].toarray(), "touched rows of A")
    # touched rows equal scipy's; every other row is A's, moved by the gain so far
    ap, cp = A.indptr.astype(np.int64), C.indptr.astype(np.int64)
    for n, r in enumerate(touched):
        _same(Cs.indices[Cs.indptr[n]:Cs.indptr[n + 1]], C.indices[cp[r]:cp[r + 1]], f"row {r} indices")
        _same(Cs.data[Cs.indptr[n]:Cs.indptr[n + 1]], C.data[cp[r]:cp[r + 1]], f"row {r} values")
        assert cp[r] == ap[r] + extra[n]
    prev = 0
    for n, r in enumerate(list(touched[:len(marked)]) + [g.pad_rows]):
        lo_, hi_ = ap[prev], ap[r]
        _same(C.indices[lo_ + extra[n]:hi_ + extra[n]], A.indices[lo_:hi_], f"untouched rows {prev}..{r} indices")
        _same(C.data[lo_ + extra[n]:hi_ + extra[n]], A.data[lo_:hi_], f"untouched rows {prev}..{r} values")
        prev = r + 1


@pytest.mark.parametrize("name", NAMES)
def test_sort_sum_input_gives_the_forward_matrix(name):
    g = geom(name)
    M, tail_want = g.build_canon_input("cpu", boundary(name))
    p, j, x = M.indptr.numpy(), M.indices.numpy(), M.values.numpy()
    assert p[-1] == M.nnz and (np.diff(p) >= 0).all()
    marked = g.marked_rows(boundary(name))
    longer = np.flatnonzero(np.diff(p[:g.pad_rows + 1]) != g.L)
    assert list(longer) == marked, "only the marked pad rows hold duplicates"
    want = cc.restate((g.rows, g.W), cc.rows_of(p), j, x, cc.SORT | cc.SUM)
    fp, fj, fx = reference(name)
    n = g.pad_nnz
    _same(want[0][:g.pad_rows + 1], fp[:g.pad_rows + 1], "pad row pointer")
    _same(want[1][:n], fj[:n], "pad indices")
    _same(want[2][:n], fx[:n], "pad values: the duplicates sum to the forward values exactly")
    _same(want[0][g.pad_rows:] - n, tail_want[0], "tail row pointer")
    _same(want[1][n:], tail_want[1], "tail indices")
    _same(want[2][n:], tail_want[2], "tail values")
    # scipy agrees with the restatement wherever its sort is stable (sum_duplicates on the tail input)
    S = cc.scipy_csr((g.rows, g.W), p, j, x)
    S.sum_duplicates()
    assert np.array_equal(S.indptr, want[0]) and np.array_equal(S.indices, want[1])
    _same(S.data[:n], fx[:n], "scipy's sums of the pad")
    # the unsorted rows are really unsorted and the tail really has duplicates
    assert not cc.scipy_csr((g.rows, g.W), p, j, x).has_sorted_indices
    assert tail_want[1].size < p[-1] - p[g.pad_rows]


@pytest.mark.parametrize("name", NAMES)
def test_sort_of_the_reversed_variant(name):
    g = geom(name)
    p, j, x = reference(name, reverse=True)
    S = cc.scipy_csr((g.rows, g.W), p, j, x)
    S.sort_indices()
    fp, fj, fx = reference(name)
    _same(S.indices, fj, "indices")
    _same(S.data, fx, "values")


@pytest.mark.parametrize("name", NAMES)
def test_dropped_zeros_model(name):
    g = geom(name)
    p, j, x = reference(name, zeros=True)
    S = cc.scipy_csr((g.rows, g.W), p, j, x)
    assert np.count_nonzero(x == 0) > 0 or g.pad_nnz < 11
    assert np.signbit(x[x == 0]).any() or g.pad_nnz < 200, "-0.0 among the zeros"
    S.eliminate_zeros()
    counts, cols, vals = zip(*[g.dropped_pad(a, b, "cpu") for a, b in g.row_slices()])
    counts = torch.cat(counts).numpy()
    n = int(counts.sum())
    assert n == g.dropped_pad_nnz() == S.indptr[g.pad_rows]
    _same(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32), S.indptr[:g.pad_rows + 1], "row pointer")
    _same(torch.cat(cols).numpy(), S.indices[:n], "indices")
    _same(torch.cat(vals).numpy(), S.data[:n], "values")
    want = cc.restate((g.rows, g.W), cc.rows_of(p), j, x, cc.DROP)
    _same(want[1], S.indices, "restate's DROP_ZEROS equals eliminate_zeros")


@pytest.mark.parametrize("name", NAMES)
def test_dense_models(name):
    g, A = geom(name), scipy_of(name)
    D = A.toarray()
    got = torch.cat([g.pad_dense(a, b, "cpu") for a, b in g.row_slices()]).numpy()
    _same(got, D[:g.pad_rows], "toarray() of the pad")
    _same(g.tail.toarray(), D[g.pad_rows:], "toarray() of the tail")
    back = sp.csr_matrix(D)
    _same(back.indices, A.indices, "csr_matrix(D) indices")
    _same(back.data, A.data, "csr_matrix(D) values")
    # with the zeros written into D: the dropped model
    p, j, x = reference(name, zeros=True)
    Z = cc.scipy_csr((g.rows, g.W), p, j, x).toarray()
    gz = torch.cat([g.pad_dense(a, b, "cpu", zeros=True) for a, b in g.row_slices()]).numpy()
    assert np.array_equal(gz, Z[:g.pad_rows])                       # (toarray() turns a stored -0.0 into 0 + -0.0 = +0.0)
    back = sp.csr_matrix(gz)
    counts, cols, vals = zip(*[g.dropped_pad(a, b, "cpu") for a, b in g.row_slices()])
    _same(torch.cat(cols).numpy(), back.indices, "indices after the zeros are dropped")
    _same(torch.cat(vals).numpy(), back.data, "values after the zeros are dropped")


@pytest.mark.parametrize("name", NAMES)
def test_coo_order_groups_back_to_the_forward_matrix(name):
    g = geom(name)
    rows, cols, vals = (t.numpy() for t in g.build_coo("cpu"))
    assert rows.size == g.nnz
    (_, o0), (_, e0) = g.coo_segments()
    assert o0 == 0 and (rows[:e0] % 2 == 1).all() and (rows[e0:] % 2 == 0).all()
    assert g.pad_rows < 2 or (np.diff(rows.astype(np.int64)) < 0).any(), "not grouped by row"
    want = sp.coo_matrix((vals, (rows, cols)), shape=(g.rows, g.W)).tocsr()     # coo_tocsr: stable
    fp, fj, fx = reference(name)
    _same(want.indptr.astype(np.int64), fp, "row pointer")
    _same(want.indices, fj, "indices")
    _same(want.data, fx, "values")
    got = cc.restate((g.rows, g.W), rows, cols, vals, 0, coo=True)
    _same(got[1], fj, "restate")


@pytest.mark.parametrize("name", NAMES)
def test_cols16_models(name):
    from spmm_amd import distributed as dist
    from spmm_amd.sparse import csr_matrix
    g = geom(name)
    M = g.build("cpu", mul=lo.WIDE_MUL, cols=lo.WIDE_COLS)
    host = csr_matrix._from_parts(M.values, M.indices, M.indptr, (g.rows, lo.WIDE_COLS), canonical=True)
    starts, lo16 = dist._cols16_split_host(host, 2)
    got = torch.cat([g.block_starts_pad(a, b, "cpu") for a, b in g.row_slices()])
    assert got.shape == (g.pad_rows, 2) and torch.equal(got, starts[:g.pad_rows])
    assert torch.equal(lo16.to(torch.int32) & 0xFFFF, M.indices & 0xFFFF)
    assert torch.equal(dist._cols16_join_host(M.indptr, starts, lo16), M.indices)


def test_full_size_arithmetic():
    f = lo.FULL
    assert f == dict(pad_rows=8589935, L=250, W=256) and f["pad_rows"] == -(-(1 << 31) // 250)
    tail = lo.make_tail(256)
    g = lo.Geometry(tail=tail, **f)                                     # (allocates nothing)
    assert g.pad_nnz == 2147483750 > 1 << 31
    s = g.straddling_row()
    assert s == 8589934 and s * g.L == 2147483500 < (1 << 31) <= 2147483749 == (s + 1) * g.L - 1
    assert g.marked_rows() == [0, 8589934, 8589935 - 1] or g.marked_rows() == [0, 8589934]
    assert g.pad_nnz + int(tail.indptr[0]) >= 1 << 31, "every tail offset is at least 2**31"
    assert g.nnz < 1 << 32 and g.rows < 1 << 24
    lens = np.diff(tail.indptr)
    assert {0, 1, 63, 64, 65, 256} <= set(lens.tolist()) and 150 < tail.shape[0] < 400
    assert (lens[6:15] == 0).all(), "a run of empty rows"
    assert lo.exactness_margin(g.L) < lo.EXACT_BOUND and lo.exactness_margin(256, 2.0, 0.5) < lo.EXACT_BOUND
    assert lo.WIDE_MUL * (g.W - 1) < lo.WIDE_COLS and -(-lo.WIDE_COLS // 65536) == 3
    need = lo.planned_bytes(g)
    for test, b in need.items():
        total = b + (need["operand"] if test != "operand" else 0)
        assert total < lo.CAP_BYTES, f"{test}: {total / lo.GiB:.1f} GiB"
    kept = g.dropped_pad_nnz()          # the zeros variant reads past 2**31 and writes below it
    assert 0.8 * g.pad_nnz < kept < 0.83 * g.pad_nnz
