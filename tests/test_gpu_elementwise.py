"""Device element-wise multiply / maximum / minimum (spg_csr_binop_nnz / spg_csr_binop), sparse times
dense per stored entry (spg_csr_mul_dense), and the containers' multiply / maximum / minimum that
run on them (cupyx's csr_matrix.multiply and _maximum_minimum,
modify_src/cupy-src/cupyx/scipy/sparse/_csr.py:328-342 and :297-326).

Bar (tests/elementwise_cases.py): C's indptr and indices equal scipy's A.multiply(B) / A.maximum(B) /
A.minimum(B) array for array, nnzC equals scipy's nnz, and the values equal scipy's under
special_values.assert_same_special -- +-0, denormals and +-inf bit for bit, NaN exactly where scipy
has one.  No entry is left out of any comparison.

Every buffer the engine writes is a tests/guarded.py buffer: poisoned with 0xFF first, C's arrays
exactly sized, guard bands around them and around the workspace checked after every run.

The kernels' seams (spmm_amd/csrc/spgemm_binop.hpp, on spgemm_geam.hpp's walk): a wave walks its
chunk of 1024 entries 64 at a time, a workgroup holds 4 waves; a step whose 64 entries lie in one
row searches a window of the other row; the three scans work in tiles of 2048.  The edge pair and
the long pair of tests/geam_cases.py reach them.

Not tested here: operands past 2**31 stored entries (SPG_STATUS_OVERFLOW, 64-bit positions in the
marks); that belongs with tests/test_gpu_large_offsets.py.
"""
import ctypes
import functools

import numpy as np
import pytest
import scipy.sparse as sp

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import elementwise_cases as ec      # noqa: E402
from tests import geam_cases as gc             # noqa: E402
from tests import special_values as sv         # noqa: E402
from tests.guarded import guarded              # noqa: E402

DTYPES = ec.DTYPES
DEV = "cuda:0"
INVALID_VALUE = 3


def _tdt(dt):
    return getattr(torch, np.dtype(dt).name)


class _Call:
    """One op(A, B) through ctypes on the scipy CSR pair (A, B), step by step, every output in a
    guarded buffer.  same: B's descriptor points at A's arrays."""

    def __init__(self, A, B, op, ip=np.int32, cp=np.int32, fill=0xFF, same=False):
        from spmm_amd import _lib
        from spmm_amd.cusparse import _IT, _VT
        self._lib, self._VT = _lib, _VT
        self.h = _lib.get_handle(0)
        self.h.set_stream(torch.cuda.current_stream(0).cuda_stream)
        self.lib, self.fill, self.op = self.h.lib, fill, ec.OP_CODE[op]
        self.shape = A.shape
        self.keep, self.bufs = [], []

        def view(S):
            p = torch.from_numpy(S.indptr.astype(ip)).to(DEV)
            j = torch.from_numpy(S.indices.astype(np.int32)).to(DEV)
            x = torch.from_numpy(S.data.copy()).to(DEV)
            self.keep += [p, j, x]
            nnz = int(S.indptr[-1])
            return _lib.SpgCsr(S.shape[0], S.shape[1], nnz, p.data_ptr(), j.data_ptr() if nnz else 0,
                               x.data_ptr() if nnz else 0, _IT[_tdt(ip)], _VT[x.dtype]), x.dtype
        self.va, self.vdt = view(A)
        self.vb = self.va if same else view(B)[0]
        self.tcp = _tdt(cp)
        self.ctype = _IT[self.tcp]
        self.cp_g = self.buf(A.shape[0] + 1, self.tcp, "C.indptr")
        self.nnz = ctypes.c_int64(-1)
        self.need = ctypes.c_size_t(0)

    def buf(self, count, dtype, name):
        g = guarded(int(count), dtype, self.fill, DEV, name)
        self.bufs.append(g)
        return g

    def query(self):
        return self.lib.spg_csr_binop_nnz(self.h.ptr, self.op, ctypes.byref(self.va), ctypes.byref(self.vb), None,
                                          self.ctype, ctypes.byref(self.nnz), ctypes.byref(self.need), None)

    def structure(self):
        self.ws = self.buf(self.need.value, torch.uint8, "workspace")
        have = ctypes.c_size_t(self.need.value)
        return self.lib.spg_csr_binop_nnz(self.h.ptr, self.op, ctypes.byref(self.va), ctypes.byref(self.vb),
                                          ctypes.c_void_p(self.cp_g.data_ptr()), self.ctype, ctypes.byref(self.nnz),
                                          ctypes.byref(have), ctypes.c_void_p(self.ws.data_ptr()))

    def values(self):
        n = int(self.nnz.value)
        self.cj, self.cx = self.buf(n, torch.int32, "C.indices"), self.buf(n, self.vdt, "C.values")
        self.vc = self._lib.SpgCsr(self.shape[0], self.shape[1], n, self.cp_g.data_ptr(), self.cj.data_ptr() if n else 0,
                                   self.cx.data_ptr() if n else 0, self.ctype, self._VT[self.vdt])
        return self.lib.spg_csr_binop(self.h.ptr, self.op, ctypes.byref(self.va), ctypes.byref(self.vb),
                                      ctypes.byref(self.vc), ctypes.c_size_t(self.need.value),
                                      ctypes.c_void_p(self.ws.data_ptr()))

    def result(self):
        torch.cuda.synchronize()
        for g in self.bufs:
            g.check()
        return self.cp_g.t.cpu().numpy(), self.cj.t.cpu().numpy(), self.cx.t.cpu().numpy()


def _run(A, B, op, ip=np.int32, cp=np.int32, fill=0xFF, same=False):
    c = _Call(A, B, op, ip, cp, fill, same)
    assert c.query() == 0 and c.need.value > 0
    assert c.structure() == 0
    assert c.values() == 0
    got = c.result()
    assert got[0].dtype == cp and int(got[0][-1]) == c.nnz.value == got[1].size == got[2].size
    return got


# ------------------------------------------------------------------ 1. edge pair
@pytest.mark.parametrize("op", ec.OPS)
@pytest.mark.parametrize("dt", DTYPES, ids=gc.case_id)
def test_edge_pair(dt, op):
    A, B = ec.pair("edge", dt)
    ec.check_categories("edge", dt, False, op)
    ref = ec.reference("edge", dt, False, op)
    got = _run(A, B, op)
    assert got[1].size == ref[1].size          # nnzC is scipy's nnz
    ec.assert_equal(got, ref)


# ------------------------------------------------------------------ 2. long pair
@pytest.mark.parametrize("op", ec.OPS)
@pytest.mark.parametrize("dt", [np.float64, np.complex64], ids=gc.case_id)
def test_long_pair(dt, op):
    """Rows of 5,000, 9,000 and 30,000 entries: longer than a wave's chunk and a workgroup's entries."""
    ec.assert_equal(_run(*ec.pair("long", dt), op), ec.reference("long", dt, False, op))


# ------------------------------------------------------------------ 3. special values
@pytest.mark.parametrize("op", ec.OPS)
@pytest.mark.parametrize("dt", DTYPES, ids=gc.case_id)
def test_special_values(dt, op):
    A, B = ec.pair("edge", dt, True)
    ec.check_categories("edge", dt, True, op)
    ref = ec.reference("edge", dt, True, op)
    assert np.isnan(ref[2].view(sv.real_dtype(dt))).sum() >= 10 and np.isinf(ref[2].view(sv.real_dtype(dt))).sum() >= 10
    ec.assert_equal(_run(A, B, op), ref)


@pytest.mark.parametrize("name,op", [(n, op) for n, (_, _, want) in ec.PROBES.items() for op in want])
def test_probes(name, op):
    A, B, _ = ec.PROBES[name]
    ec.check_probe(name, op, _run(A, B, op))


# ------------------------------------------------------------------ 4. index widths
@pytest.mark.parametrize("op", ["multiply", "maximum"])
def test_index_widths(op):
    A, B = ec.pair("edge", np.float64)
    base = _run(A, B, op)
    ec.assert_equal(base, ec.reference("edge", np.float64, False, op))
    for ip, cp in [(np.int64, np.int64), (np.int32, np.int64), (np.int64, np.int32)]:
        got = _run(A, B, op, ip=ip, cp=cp)
        assert got[0].dtype == cp and np.array_equal(got[0], base[0]) and np.array_equal(got[1], base[1])
        assert np.array_equal(got[2].view(np.uint8), base[2].view(np.uint8))


# ------------------------------------------------------------------ 5. degenerate sizes
@pytest.mark.parametrize("op", ec.OPS)
@pytest.mark.parametrize("shape", [(0, 0), (0, 5)])
def test_no_rows(shape, op):
    from spmm_amd import _lib
    E = sp.csr_matrix(shape, dtype=np.float64)
    h = _lib.get_handle(0)
    h.set_timing(True)
    try:
        p, j, x = _run(E, E, op)
        launches = h.get_timing()
    finally:
        h.set_timing(False)
    assert p.tolist() == [0] and j.size == 0 and x.size == 0
    assert all(n == 0 for _, n in launches.values())          # rows == 0 launches nothing


@pytest.mark.parametrize("op", ec.OPS)
@pytest.mark.parametrize("dt", [np.float32, np.complex128], ids=gc.case_id)
@pytest.mark.parametrize("empty", ["A", "B", "both"])
def test_empty_operands(empty, dt, op):
    """An operand without entries still evaluates the other one against 0: 0 * inf is NaN and is
    stored under multiply."""
    A, B = ec.pair("edge", dt, True)
    Z = sp.csr_matrix(A.shape, dtype=dt)
    A, B = (Z if empty in ("A", "both") else A), (Z if empty in ("B", "both") else B)
    ref = ec.scipy_binop(A, B, op)
    got = _run(A, B, op)
    ec.assert_equal(got, ref)
    if empty == "both":
        assert not got[0].any() and got[1].size == 0
    elif op == "multiply":
        assert got[2].size >= 10 and np.isnan(got[2].view(sv.real_dtype(dt)).reshape(got[2].size, -1)).any(axis=1).all()
    else:
        assert got[2].size >= 100


def test_disjoint_patterns_give_an_empty_product():
    """Interleaved finite patterns under multiply: nnzC == 0 and the value call launches nothing."""
    from spmm_amd import _lib
    rng = np.random.default_rng(3)
    m, n = 300, 257
    ev = sp.random(m, n // 2 + 1, density=0.2, random_state=rng, format="coo")
    od = sp.random(m, n // 2, density=0.2, random_state=rng, format="coo")
    A = sp.csr_matrix((ev.data + 1, (ev.row, 2 * ev.col)), shape=(m, n))
    B = sp.csr_matrix((od.data + 1, (od.row, 2 * od.col + 1)), shape=(m, n))
    A.sort_indices(), B.sort_indices()
    assert A.nnz > 4096 and B.nnz > 4096 and A.multiply(B).nnz == 0
    c = _Call(A, B, "multiply")
    assert c.query() == 0 and c.structure() == 0 and c.nnz.value == 0
    c.h.set_timing(True)
    try:
        assert c.values() == 0
        p, j, x = c.result()
        launches = c.h.get_timing()
    finally:
        c.h.set_timing(False)
    assert not p.any() and p.size == m + 1 and j.size == 0 and x.size == 0
    assert all(k == 0 for _, k in launches.values())
    for op in ("maximum", "minimum"):          # the same pair keeps its one-sided entries under the other two
        ec.assert_equal(_run(A, B, op), ec.scipy_binop(A, B, op))


@pytest.mark.parametrize("op", ec.OPS)
@pytest.mark.parametrize("dt", DTYPES, ids=gc.case_id)
def test_same_arrays(dt, op):
    """op(A, A) with B's descriptor pointing at A's arrays."""
    A, _ = ec.pair("edge", dt, True)
    ec.assert_equal(_run(A, A, op, same=True), ec.scipy_binop(A, A, op))


# ------------------------------------------------------------------ 6. determinism
@pytest.mark.parametrize("op", ec.OPS)
def test_runs_are_identical(op):
    """The same bytes in all three arrays from one run to the next, and with the workspace and the
    outputs pre-filled with 0x00 instead of 0xFF: nothing stale is read."""
    A, B = ec.pair("edge", np.complex64, True)
    runs = [_run(A, B, op, fill=f) for f in (0xFF, 0xFF, 0x00)]
    ec.assert_equal(runs[0], ec.reference("edge", np.complex64, True, op))
    for r in runs[1:]:
        for a, b in zip(r, runs[0]):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ------------------------------------------------------------------ 7. spg_csr_mul_dense
def _noncanonical(dt):
    """The edge matrix with every row reversed (unsorted) and its first 300 entries stored twice."""
    A, _ = ec.pair("edge", dt, True)
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    order = np.lexsort((-A.indices, rows))
    r, j, x = rows[order], A.indices[order], A.data[order]
    r, j, x = np.concatenate([r[:300], r]), np.concatenate([j[:300], j]), np.concatenate([x[:300], x])
    o = np.argsort(r, kind="stable")
    indptr = np.zeros(A.shape[0] + 1, dtype=np.int32)
    indptr[1:] = np.cumsum(np.bincount(r, minlength=A.shape[0]))
    N = sp.csr_matrix((x[o], j[o], indptr), shape=A.shape)
    assert not N.has_canonical_format and N.nnz == A.nnz + 300
    return N


def _mul_dense(A, D_dev, view, ip=np.int32, in_place=False):
    """spg_csr_mul_dense through ctypes: (status, values, A's arrays afterwards)."""
    from spmm_amd import _lib
    from spmm_amd.cusparse import _IT, _VT
    h = _lib.get_handle(0)
    h.set_stream(torch.cuda.current_stream(0).cuda_stream)
    p = torch.from_numpy(A.indptr.astype(ip)).to(DEV)
    j = torch.from_numpy(A.indices.astype(np.int32)).to(DEV)
    nnz = int(A.indptr[-1])
    gx = guarded(nnz, A.dtype, 0xFF, DEV, "A.values")
    gx.t.copy_(torch.from_numpy(A.data.copy()))
    out = gx if in_place else guarded(nnz, A.dtype, 0xFF, DEV, "out")
    va = _lib.SpgCsr(A.shape[0], A.shape[1], nnz, p.data_ptr(), j.data_ptr() if nnz else 0, gx.data_ptr() if nnz else 0,
                     _IT[_tdt(ip)], _VT[gx.t.dtype])
    rows, cols, ld, order = view
    vd = _lib.SpgDense(rows, cols, ld, D_dev.data_ptr(), order, _VT[gx.t.dtype])
    st = h.lib.spg_csr_mul_dense(h.ptr, ctypes.byref(va), ctypes.byref(vd), ctypes.c_void_p(out.data_ptr()))
    torch.cuda.synchronize()
    gx.check(), out.check()
    assert np.array_equal(p.cpu().numpy(), A.indptr) and np.array_equal(j.cpu().numpy(), A.indices)   # structure untouched
    if not in_place:
        assert np.array_equal(gx.t.cpu().numpy().view(np.uint8), A.data.view(np.uint8))
    return st, out.t.cpu().numpy()


def _layouts(D):
    """(name, device tensor, (rows, cols, ld, order)) of D row-major, column-major and with a padded ld."""
    from spmm_amd import _lib
    r, c = D.shape
    t = torch.from_numpy(D.copy()).to(DEV)
    wide = torch.full((r, c + 3), float("nan"), dtype=t.dtype, device=DEV)
    wide[:, :c] = t
    return [("row", t, (r, c, c, _lib.SPG_ORDER_ROW)), ("col", t.t().contiguous(), (r, c, r, _lib.SPG_ORDER_COL)),
            ("padded", wide, (r, c, c + 3, _lib.SPG_ORDER_ROW))]


@pytest.mark.parametrize("which", ["full", "row", "col", "one"])
@pytest.mark.parametrize("dt", DTYPES, ids=gc.case_id)
def test_mul_dense(dt, which):
    A, _ = ec.pair("edge", dt, True)
    m, n = A.shape
    D = ec.dense_operand(np.random.default_rng(11), {"full": (m, n), "row": (1, n), "col": (m, 1), "one": (1, 1)}[which], dt)
    want = ec.mul_dense_reference(A, D)
    assert (want == 0).sum() >= 10                      # products that are zero stay stored
    for name, t, view in _layouts(D):
        st, got = _mul_dense(A, t, view)
        assert st == 0, name
        sv.assert_values_special(got, want, f"{which} {name}")


@pytest.mark.parametrize("dt", DTYPES, ids=gc.case_id)
def test_mul_dense_noncanonical_int64_in_place(dt):
    from spmm_amd import _lib
    N = _noncanonical(dt)
    m, n = N.shape
    D = ec.dense_operand(np.random.default_rng(12), (m, n), dt)
    want = ec.mul_dense_reference(N, D)
    if np.dtype(dt).kind != "c":        # scipy keeps every stored entry in stored order (as COO)
        with np.errstate(all="ignore"):
            R = N.multiply(D).tocoo()
        assert np.array_equal(R.col, N.indices)
        sv.assert_values_special(R.data, want)
    t = torch.from_numpy(D.copy()).to(DEV)
    view = (m, n, n, _lib.SPG_ORDER_ROW)
    for ip, in_place in [(np.int32, False), (np.int64, False), (np.int64, True), (np.int32, True)]:
        st, got = _mul_dense(N, t, view, ip=ip, in_place=in_place)
        assert st == 0
        sv.assert_values_special(got, want, f"ip={np.dtype(ip).name} in_place={in_place}")


def test_mul_dense_statuses_and_empty():
    from spmm_amd import _lib
    A, _ = ec.pair("edge", np.float64)
    m, n = A.shape
    t = torch.ones((m + 1, n + 1), dtype=torch.float64, device=DEV)
    R, C = _lib.SPG_ORDER_ROW, _lib.SPG_ORDER_COL
    for view in [(m + 1, n, n + 1, R), (m, n + 1, n + 1, R), (2, n, n + 1, R), (m, n, n - 1, R), (m, n, m - 1, C),
                 (m, n, n + 1, 7)]:
        assert _mul_dense(A, t, view)[0] == INVALID_VALUE, view
    Z = sp.csr_matrix(A.shape, dtype=np.float64)
    h = _lib.get_handle(0)
    h.set_timing(True)
    try:
        st, got = _mul_dense(Z, t, (m, n, n + 1, R))
        launches = h.get_timing()
    finally:
        h.set_timing(False)
    assert st == 0 and got.size == 0 and all(k == 0 for _, k in launches.values())


# ------------------------------------------------------------------ 8. the Python layer
def _parts(m):
    torch.cuda.synchronize()
    return m.indptr.cpu().numpy(), m.indices.cpu().numpy(), m.data.cpu().numpy()


def _csr_parts(m):
    torch.cuda.synchronize()
    S = m.get().tocsr()
    S.sort_indices()
    return S.indptr, S.indices, S.data


def _dev(S, fmt="csr"):
    from spmm_amd.sparse import coo_matrix, csc_matrix, csr_matrix
    return {"csr": csr_matrix, "csc": csc_matrix, "coo": coo_matrix}[fmt](S, device=DEV)


@pytest.mark.parametrize("op", ec.OPS)
@pytest.mark.parametrize("dt", DTYPES, ids=gc.case_id)
def test_methods(dt, op):
    from spmm_amd import _lib, cusparse
    assert cusparse.has_elementwise() is True
    A, B = ec.pair("edge", dt, True)
    ref = ec.reference("edge", dt, True, op)
    dA, dB = _dev(A), _dev(B)
    h = _lib.get_handle(0)
    h.set_timing(True)
    try:
        C = getattr(dA, op)(dB)
        torch.cuda.synchronize()
        launches = h.get_timing()
    finally:
        h.set_timing(False)
    assert launches["numeric"][1] == 1 and launches["symbolic"][1] == 2 and launches["scan"][1] == 3   # the engine ran
    assert C.format == "csr" and C._canonical is True and C.shape == A.shape and C.indptr.dtype == torch.int32
    ec.assert_equal(_parts(C), ref)
    ec.assert_equal(_parts(cusparse.csrbinop(dA, dB, op)), ref)
    for fa, fb in [("csc", "csc"), ("csr", "csc"), ("csc", "coo"), ("coo", "csr"), ("coo", "coo")]:
        C = getattr(_dev(A, fa), op)(_dev(B, fb))
        assert C.format == ("csc" if fa == "csc" else "csr") and C.shape == A.shape and C._canonical is True
        ec.assert_equal(_csr_parts(C), ref)


def test_product_masked_by_its_operand():
    """(A @ A).multiply(A): the triangle-counting mask."""
    from tests.golden_cases import load
    A, _, _, _ = load("config1_n1024_d0.01_f64")
    dA = _dev(A)
    got = (dA @ dA).multiply(dA)
    P = A @ A
    P.sort_indices()
    ec.assert_equal(_parts(got), ec.scipy_binop(P.tocsr(), A, "multiply"))
    assert got.nnz > 0


@pytest.mark.parametrize("dt", [np.float32, np.complex128], ids=gc.case_id)
def test_row_and_column_scaling(dt):
    """D_r A D_c: A.multiply(d_row).multiply(d_col), for csr, csc and coo containers; numpy and device
    operands; promotion; scalars."""
    from spmm_amd import _lib, cusparse
    A, _ = ec.pair("edge", dt, True)
    m, n = A.shape
    rng = np.random.default_rng(13)
    d_row, d_col = ec.dense_operand(rng, (m, 1), dt), ec.dense_operand(rng, (n,), dt)
    step = sp.csr_matrix((ec.mul_dense_reference(A, d_row), A.indices, A.indptr), shape=A.shape)
    want = ec.mul_dense_reference(step, d_col)
    h = _lib.get_handle(0)
    for fmt in ("csr", "csc", "coo"):
        dA = _dev(A, fmt)
        h.set_timing(True)
        try:
            got = dA.multiply(d_row).multiply(torch.from_numpy(d_col.copy()).to(DEV))
            torch.cuda.synchronize()
            launches = h.get_timing()
        finally:
            h.set_timing(False)
        # one spg_csr_mul_dense launch each (for coo the conversion to csr runs a value kernel of its own)
        assert launches["numeric"][1] == 2 if fmt != "coo" else launches["numeric"][1] >= 2
        assert got.format == ("csc" if fmt == "csc" else "csr") and got._canonical is True
        sv.assert_same_special(_csr_parts(got), (A.indptr, A.indices, want))
    got = cusparse.multiply_by_dense(_dev(A), d_row)
    sv.assert_same_special(_parts(got), (A.indptr, A.indices, step.data))
    s = _dev(A) * 2.5
    sv.assert_same_special(_parts(s), (A.indptr, A.indices, sv.cmul(2.5, A.data)))
    sv.assert_same_special(_parts((0.5 + 2j) * _dev(A)), (A.indptr, A.indices, sv.cmul(0.5 + 2j, A.data.astype(
        np.result_type(dt, 1j)))))


def test_clipping_and_errors():
    """C.maximum(0 * C) clips at zero; shapes that differ and dense operands of maximum are refused."""
    A, B = ec.pair("edge", np.float64)
    dA = _dev(A)
    got = dA.maximum(0 * dA)
    with np.errstate(all="ignore"):
        ec.assert_equal(_parts(got), ec.scipy_binop(A, (0 * A).tocsr(), "maximum"))
    assert (got.data > 0).all() and 0 < got.nnz < A.nnz
    with pytest.raises(NotImplementedError, match="different shapes"):
        dA.multiply(_dev(sp.csr_matrix((1, A.shape[1]), dtype=np.float64)))
    with pytest.raises(NotImplementedError, match="maximum with a scalar or a dense operand"):
        dA.maximum(torch.zeros(A.shape, device=DEV))
    with pytest.raises(TypeError, match="expected scalar, dense matrix/vector or csr matrix"):
        dA.multiply("abc")


# ------------------------------------------------------------------ 9. timing
def test_phases():
    """With timing on, one binop adds launches only under symbolic (mark, count), scan (three) and
    numeric (fill); the size query launches nothing; one spg_csr_mul_dense adds exactly one launch
    under numeric."""
    from spmm_amd import _lib
    A, B = ec.pair("edge", np.float64)
    c = _Call(A, B, "minimum")
    c.h.set_timing(True)
    try:
        assert c.query() == 0 and c.need.value > 0
        after_query = c.h.get_timing()
        assert c.structure() == 0
        after_nnz = c.h.get_timing()
        assert c.values() == 0
        got = c.result()
        after = c.h.get_timing()
    finally:
        c.h.set_timing(False)
    assert all(n == 0 for _, n in after_query.values())
    assert after_nnz["symbolic"][1] == 2 and after_nnz["scan"][1] == 3 and after_nnz["numeric"][1] == 0
    assert after["numeric"][1] == 1 and after["symbolic"][1] == 2 and after["scan"][1] == 3
    assert all(n == 0 for k, (_, n) in after.items() if k not in ("symbolic", "scan", "numeric"))
    assert len(_lib.PHASES) == 9 and len(after) == 9
    ec.assert_equal(got, ec.reference("edge", np.float64, False, "minimum"))
    D = np.ones(A.shape)
    c.h.set_timing(True)
    try:
        st, _ = _mul_dense(A, torch.from_numpy(D).to(DEV), (*A.shape, A.shape[1], _lib.SPG_ORDER_ROW))
        after = c.h.get_timing()
    finally:
        c.h.set_timing(False)
    assert st == 0 and after["numeric"][1] == 1
    assert all(n == 0 for k, (_, n) in after.items() if k != "numeric")


def test_null_and_mismatched_arguments():
    from spmm_amd import _lib
    A, B = gc.random_pair(70, 33, 500, 400)
    c = _Call(A, B, "multiply")
    lib, h = c.lib, c.h.ptr
    a, b, nnz, need = ctypes.byref(c.va), ctypes.byref(c.vb), ctypes.byref(c.nnz), ctypes.byref(c.need)
    assert lib.spg_csr_binop_nnz(h, 0, None, b, None, c.ctype, nnz, need, None) == INVALID_VALUE
    assert lib.spg_csr_binop_nnz(h, 0, a, None, None, c.ctype, nnz, need, None) == INVALID_VALUE
    assert lib.spg_csr_binop_nnz(h, 0, a, b, None, c.ctype, None, need, None) == INVALID_VALUE
    assert lib.spg_csr_binop_nnz(h, 0, a, b, None, c.ctype, nnz, None, None) == INVALID_VALUE
    assert lib.spg_csr_binop_nnz(h, 0, a, b, None, 16, nnz, need, None) == INVALID_VALUE      # bad C_indptr_type
    assert lib.spg_csr_binop_nnz(h, 5, a, b, None, c.ctype, nnz, need, None) == INVALID_VALUE   # unknown op
    assert c.query() == 0
    ws = c.buf(c.need.value, torch.uint8, "ws")
    short = ctypes.c_size_t(c.need.value - 1)
    wsp, cpp = ctypes.c_void_p(ws.data_ptr()), ctypes.c_void_p(c.cp_g.data_ptr())
    assert lib.spg_csr_binop_nnz(h, 0, a, b, None, c.ctype, nnz, need, wsp) == INVALID_VALUE   # NULL C_indptr with a workspace
    assert lib.spg_csr_binop_nnz(h, 0, a, b, cpp, c.ctype, nnz, ctypes.byref(short), wsp) == INVALID_VALUE
    c.vb.cols += 1
    assert c.query() == INVALID_VALUE
    c.vb.cols -= 1
    c.vb.value_type = _lib.SPG_R_32F
    assert c.query() == INVALID_VALUE
    c.vb.value_type = c.va.value_type
    assert c.structure() == 0 and c.values() == 0
    n, wsp = ctypes.c_size_t(c.need.value), ctypes.c_void_p(c.ws.data_ptr())
    vc = ctypes.byref(c.vc)
    assert lib.spg_csr_binop(h, 0, a, b, None, n, wsp) == INVALID_VALUE
    assert lib.spg_csr_binop(h, 0, a, b, vc, n, None) == INVALID_VALUE
    assert lib.spg_csr_binop(h, 0, a, b, vc, ctypes.c_size_t(c.need.value - 1), wsp) == INVALID_VALUE
    assert lib.spg_csr_binop(h, 9, a, b, vc, n, wsp) == INVALID_VALUE
    c.vc.rows += 1
    assert lib.spg_csr_binop(h, 0, a, b, vc, n, wsp) == INVALID_VALUE
    c.vc.rows -= 1
    assert lib.spg_csr_binop(h, 0, a, b, vc, n, wsp) == 0
    ec.assert_equal(c.result(), ec.scipy_binop(A, B, "multiply"))
