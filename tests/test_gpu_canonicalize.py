"""Device canonicalisation (spg_canonicalize_nnz / spg_canonicalize, include/spgemm.h) and the
container methods and operators that run on it.

Bar: tests/canon_cases.py's `restate` (a stable lexsort by (row, column), every run of equal cells
summed left to right in stored order from a copy of its first value, `!= 0` for the drop), pinned to
scipy in tests/test_canon_cpu.py.  indptr and indices must be equal, values equal under
special_values.assert_same_special (NaN exactly where the reference has one, every other component
bit-equal).

The kernels' seams (spmm_amd/csrc/spgemm_canon.hpp, spgemm_transpose.hpp): a wave sorts its chunk of
TR_CHUNK = 2048 entries 64 at a time, a workgroup holds TR_WPB = 4 waves (8192 entries); the sort key
is row << bits(cols - 1) | column, 32 bits wide when it fits and 64 otherwise, sorted in 8-bit digit
passes; the mark and value kernels run 256 sorted entries per workgroup and a run's head walks the
whole run, whoever owns its tail.

Not tested here: SPG_STATUS_OVERFLOW (nnz(C) past an int32 row pointer) needs 2**31 entries;
tests/test_gpu_large_offsets.py::test_canonicalize_sort_sum has them, built on the device.
"""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import canon_cases as cc          # noqa: E402
from tests import special_values as sv       # noqa: E402

DTYPES = cc.DTYPES
SORT, SUM, DROP = cc.SORT, cc.SUM, cc.DROP
IPCP = [(np.int32, np.int32), (np.int32, np.int64), (np.int64, np.int32), (np.int64, np.int64)]
OPS = [0, SORT, SUM, DROP, SUM | DROP]
INVALID_VALUE = 3
DEV = "cuda:0"
SLACK = 8          # poisoned entries kept past every output


def _ipcp_id(v):
    return "A%d-C%d" % (np.dtype(v[0]).itemsize * 8, np.dtype(v[1]).itemsize * 8)


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint8)


class _Call:
    """One canonicalisation through ctypes, step by step.  The input is the triplets as COO
    (coo=True) or their CSR form with every row in stored order.  The workspace and the three
    output arrays hold 0xFF bytes before the calls."""

    def __init__(self, shape, rows, cols, vals, ops, coo, ip=np.int32, cp=np.int32):
        from spmm_amd import _lib
        from spmm_amd.cusparse import _IT, _VT
        self.mod = _lib
        self.h = _lib.get_handle(0)
        self.h.set_stream(torch.cuda.current_stream(0).cuda_stream)
        self.lib = self.h.lib
        self.shape, self.ops, self.coo = (int(shape[0]), int(shape[1])), ops, coo
        m, n = self.shape
        vals = np.asarray(vals)
        self.nnz_in = vals.size
        tip = torch.int32 if ip == np.int32 else torch.int64
        self.tcp = torch.int32 if cp == np.int32 else torch.int64
        if coo:
            p, j, x = None, np.asarray(cols), vals
            self.rows_t = torch.from_numpy(np.asarray(rows).astype(np.int32)).to(DEV)
        else:
            p, j, x = cc.as_csr(m, rows, cols, vals)
            self.rows_t = None
        self.ref_in = (cc.rows_of(p) if p is not None else np.asarray(rows), j, x)
        self.p_t = torch.from_numpy(p.astype(ip)).to(DEV) if p is not None else None
        self.j_t = torch.from_numpy(np.asarray(j).astype(np.int32)).to(DEV)
        self.x_t = torch.from_numpy(np.array(x, copy=True)).to(DEV)
        self.vdt = self.x_t.dtype
        nz = self.nnz_in
        self.va = _lib.SpgCsr(m, n, nz, self.p_t.data_ptr() if p is not None else 0, self.j_t.data_ptr() if nz else 0,
                              self.x_t.data_ptr() if nz else 0, _IT[tip], _VT[self.vdt])
        self.rows_p = ctypes.c_void_p(self.rows_t.data_ptr() if nz else 8) if coo else None   # (8: non-NULL, never read)
        self.ctype, self._VT = _IT[self.tcp], _VT
        self.cp_t = self.buf(m + 1 + SLACK, self.tcp)
        self.nnz = ctypes.c_int64(-1)
        self.need = ctypes.c_size_t(0)
        self.ws = self.vc = None

    def reference(self):
        return cc.restate(self.shape, *self.ref_in, self.ops, coo=self.coo)

    @staticmethod
    def buf(count, dtype):
        t = torch.empty(max(int(count), 1), dtype=dtype, device=DEV)
        t.view(torch.uint8).fill_(0xFF)
        return t

    def query(self):
        return self.lib.spg_canonicalize_nnz(self.h.ptr, ctypes.byref(self.va), self.rows_p, self.ops, None,
                                             self.ctype, ctypes.byref(self.nnz), ctypes.byref(self.need), None)

    def structure(self, shrink=0):
        self.ws = self.buf(self.need.value, torch.uint8)
        have = ctypes.c_size_t(self.need.value - shrink)
        return self.lib.spg_canonicalize_nnz(self.h.ptr, ctypes.byref(self.va), self.rows_p, self.ops,
                                             ctypes.c_void_p(self.cp_t.data_ptr()), self.ctype,
                                             ctypes.byref(self.nnz), ctypes.byref(have),
                                             ctypes.c_void_p(self.ws.data_ptr()))

    def values(self):
        n = int(self.nnz.value)
        self.cj, self.cx = self.buf(n + SLACK, torch.int32), self.buf(n + SLACK, self.vdt)
        self.vc = self.mod.SpgCsr(self.shape[0], self.shape[1], n, self.cp_t.data_ptr(), self.cj.data_ptr(),
                                  self.cx.data_ptr(), self.ctype, self._VT[self.vdt])
        return self.lib.spg_canonicalize(self.h.ptr, ctypes.byref(self.va), self.rows_p, self.ops,
                                         ctypes.byref(self.vc), ctypes.c_size_t(self.need.value),
                                         ctypes.c_void_p(self.ws.data_ptr()))

    def result(self):
        """(indptr, indices, data); nothing past them was written."""
        torch.cuda.synchronize()
        n, m = int(self.nnz.value), self.shape[0]
        p, j, x = self.cp_t.cpu().numpy(), self.cj.cpu().numpy(), self.cx.cpu().numpy()
        for tail in (p[m + 1:], j[n:], x[n:]):
            assert tail.size == SLACK and (_bits(tail) == 0xFF).all(), "written past the result"
        return p[:m + 1], j[:n], x[:n]


def _run(shape, rows, cols, vals, ops, coo, ip=np.int32, cp=np.int32, check=True):
    c = _Call(shape, rows, cols, vals, ops, coo, ip, cp)
    assert c.query() == 0 and c.need.value > 0
    assert c.structure() == 0
    assert c.values() == 0
    got = c.result()
    assert got[0].dtype == cp and int(got[0][-1]) == c.nnz.value
    if check:
        sv.assert_same_special(got, c.reference())
    return got


def _forms(ops):
    return [True] if ops == 0 else [False, True]


def _mixed_input(dt, seed):
    """Unsorted triplets with duplicates of any multiplicity, stored zeros and cells that cancel."""
    m, n = 70, 310
    rows, cols, vals = cc.pool_triplets(m, 300, 5000, 2000, dt, seed)
    vals[::9] = 0
    rng = np.random.default_rng(seed + 1)
    er, ec = rng.integers(0, m, 40), 300 + rng.integers(0, 10, 40)
    key = np.unique(er * n + ec)
    er, ec = key // n, key % n
    ev = cc.draw_values(rng, er.size, dt)
    rows, cols, vals = (np.concatenate(a) for a in ((rows, er, er), (cols, ec, ec), (vals, ev, -ev)))
    perm = rng.permutation(vals.size)
    return (m, n), rows[perm], cols[perm], vals[perm]


# ------------------------------------------------------------------ 1. every op, form, type and width
@pytest.mark.parametrize("ipcp", IPCP, ids=_ipcp_id)
@pytest.mark.parametrize("name", list(DTYPES))
def test_every_op_and_form(name, ipcp):
    shape, rows, cols, vals = _mixed_input(DTYPES[name], seed=100)
    sizes = {}
    for ops in OPS:
        for coo in _forms(ops):
            got = _run(shape, rows, cols, vals, ops, coo, *ipcp)
            sizes[ops, coo] = got[1].size
    assert sizes[SORT, True] == sizes[0, True] == vals.size
    assert sizes[SUM | DROP, True] < sizes[SUM, True] < vals.size      # duplicates summed, cancelled sums dropped
    assert sizes[DROP, False] < vals.size


# ------------------------------------------------------------------ 2. seams
@pytest.mark.parametrize("nnz", [0, 1, 63, 64, 65, 2047, 2048, 2049, 8191, 8192, 8193])
def test_entry_count_seams(nnz):
    m, n = 50, 50
    rows, cols, vals = cc.pool_triplets(m, n, nnz, nnz // 2 + 1, np.float64, seed=200 + nnz)
    for ops in (SUM, SORT, DROP):
        for coo in (False, True):
            if nnz == 0:
                c = _Call((m, n), rows, cols, vals, ops, coo)
                assert c.query() == 0 and c.structure() == 0 and c.nnz.value == 0
                torch.cuda.synchronize()
                assert not c.cp_t[:m + 1].cpu().numpy().any()
            else:
                _run((m, n), rows, cols, vals, ops, coo)


@pytest.mark.parametrize("m,n", [(1, 300), (255, 300), (256, 300), (257, 300), (65536, 300), (65537, 300),
                                 (300, 1), (300, 255), (300, 256), (300, 257), (300, 65536), (300, 65537),
                                 (65536, 65536), (65536, 65537), (65537, 65537)])
def test_shape_seams_pass_counts(m, n):
    """The key is bits(rows - 1) + bits(cols - 1) wide, 2 through 34 bits here: one to five digit
    passes, a last digit of one to eight bits, and both key widths (32 bits up to 65536 x 65536, 64
    from 65536 x 65537 on)."""
    rows, cols, vals = cc.pool_triplets(m, n, 4000, 1500, np.float64, seed=300)
    rows[:4], cols[:4] = [0, m - 1, 0, m - 1], [0, n - 1, n - 1, 0]          # the corners
    for coo in (False, True):
        got = _run((m, n), rows, cols, vals, SUM, coo)
        assert got[1][-1] == n - 1 and int(got[0][-2]) < int(got[0][-1])     # the last cell is there
    _run((m, n), rows, cols, vals, 0, True)


def test_empty_rows_and_one_full_row():
    m, n = 40, 500
    rows, cols, vals = cc.pool_triplets(m, n, 3000, 1200, np.float32, seed=400)
    rows = 5 + rows % 20                  # rows 0-4 and 25-39 empty
    rows[rows == 12] = 13                 # and row 12, in the middle
    for ops in OPS:
        for coo in _forms(ops):
            got = _run((m, n), rows, cols, vals, ops, coo)
            p = got[0]
            assert p[5] == 0 and p[12] == p[13] and p[25] == p[-1]
    for ops in OPS:
        for coo in _forms(ops):
            _run((m, n), np.full_like(rows, 17), cols, vals, ops, coo)   # one row holds everything


# ------------------------------------------------------------------ 3. runs of duplicates
def _runs_across(dt, seed=500):
    """Distinct cells in sorted order with a run of 21 equal cells over sorted entries 2038..2058
    (a wave chunk boundary at 2048) and another over 8182..8202 (a workgroup boundary at 8192),
    stored in shuffled order."""
    m, n = 6, 4000
    keys = np.sort(np.random.default_rng(seed).choice(m * n, 9000, replace=False))
    reps = np.ones(keys.size, dtype=np.int64)
    reps[2038] = 21                                   # sorted entries 2038 .. 2058
    reps[8182 - 20] = 21                              # 20 entries later in sorted order: 8182 .. 8202
    keys = np.repeat(keys, reps)
    assert keys[2038] == keys[2058] != keys[2059] and keys[2037] != keys[2038]
    assert keys[8182] == keys[8202] != keys[8203] and keys[8181] != keys[8182]
    rng = np.random.default_rng(seed + 1)
    vals = cc.draw_values(rng, keys.size, dt)
    perm = rng.permutation(keys.size)
    return (m, n), (keys // n)[perm], (keys % n)[perm], vals[perm]


@pytest.mark.parametrize("name", list(DTYPES))
def test_runs_across_chunk_and_workgroup_boundaries(name):
    shape, rows, cols, vals = _runs_across(DTYPES[name])
    for coo in (False, True):
        _run(shape, rows, cols, vals, SUM, coo)
        _run(shape, rows, cols, vals, SUM | DROP, coo)


@pytest.mark.parametrize("name", list(DTYPES))
def test_one_cell_of_3000_entries(name):
    """One run over two wave chunks, one lane's loop; values over 12 decades, so the order shows."""
    dt = DTYPES[name]
    rng = np.random.default_rng(600)
    vals = cc.draw_values(rng, 3000, dt)
    rows, cols = np.full(3000, 2), np.full(3000, 7)
    rows[:5], cols[:5] = [0, 4, 2, 2, 1], [1, 9, 6, 8, 7]                   # a few other cells around it
    fwd = cc.restate((5, 10), rows, cols, vals, SUM, coo=True)
    rev = cc.restate((5, 10), rows[::-1], cols[::-1], vals[::-1], SUM, coo=True)
    assert not np.array_equal(_bits(fwd[2]), _bits(rev[2]))                  # the order of addition matters here
    for coo in (False, True):
        got = _run((5, 10), rows, cols, vals, SUM, coo)
        assert got[1].size == 6


def test_multiplicity_two_everywhere_matches_scipy():
    m, n = 200, 300
    rows, cols, vals = cc.mult2_triplets(m, n, 6000, 1.0, np.float64, seed=700)
    got = _run((m, n), rows, cols, vals, SUM, False)
    assert 2 * got[1].size == vals.size
    S = cc.scipy_csr((m, n), *cc.as_csr(m, rows, cols, vals))
    S.sum_duplicates()
    sv.assert_same_special(got, (S.indptr, S.indices, S.data))


def test_adjacent_and_scattered_duplicates():
    m, n = 30, 200
    rows, cols, vals = cc.pool_triplets(m, n, 5000, 1500, np.float64, seed=800)
    scattered = _run((m, n), rows, cols, vals, SUM, False)
    order = np.lexsort((cols, rows))                     # sorted rows: the duplicates sit side by side
    adjacent = _run((m, n), rows[order], cols[order], vals[order], SUM, False)
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(scattered, adjacent))
    _run((m, n), rows[order], cols[order], vals[order], SORT, False)


# ------------------------------------------------------------------ 4. stored order
@pytest.mark.parametrize("name", list(DTYPES))
def test_each_stored_order_gets_its_own_sum(name):
    a, b = cc.order_pair(DTYPES[name])               # (asserts on the CPU that the two sums differ)
    for coo in (False, True):
        ga = _run(*a, SUM, coo)
        gb = _run(*b, SUM, coo)
        assert np.array_equal(ga[1], gb[1]) and not np.array_equal(_bits(ga[2]), _bits(gb[2]))


# ------------------------------------------------------------------ 5. special values
def _nan_with_payload(rd):
    bits = {np.dtype(np.float32): (np.uint32, 0x7FC12345), np.dtype(np.float64): (np.uint64, 0xFFF8000000ABCDEF)}
    t, b = bits[np.dtype(rd)]
    return np.array([b], dtype=t).view(rd)[0]


@pytest.mark.parametrize("name", list(DTYPES))
def test_special_values(name):
    dt = DTYPES[name]
    rd = sv.real_dtype(dt)
    den = np.finfo(rd).smallest_subnormal
    cx = np.dtype(dt).kind == "c"

    def val(re, im=0.0):
        if not cx:
            return np.array([re], dtype=dt)[0]
        out = np.empty(1, dtype=dt)
        out.real, out.imag = re, im
        return out[0]
    nan = _nan_with_payload(rd)
    singles = [val(-0.0, -0.0), val(den, -den), val(np.inf, -np.inf), val(-np.inf, 1.0), val(nan, 2.0),
               val(0.0, den if cx else 0.0), val(0.0, -0.0), val(3.0, -0.0)]
    # row 0: single entries; row 1: duplicated cells
    trip = [(0, 2 * k + 1, v) for k, v in enumerate(singles)]
    trip += [(1, 4, val(np.inf, 1.0)), (1, 4, val(-np.inf, 1.0)),              # inf + -inf: NaN
             (1, 2, val(1.5, -2.5)), (1, 2, val(-1.5, 2.5)),                   # x + -x: 0.0
             (1, 9, val(den, den)), (1, 9, val(den, den)),                     # a denormal sum
             (1, 6, val(-0.0, -0.0)), (1, 6, val(-0.0, -0.0))]                 # -0.0 + -0.0: -0.0
    perm = np.random.default_rng(900).permutation(len(trip))
    rows, cols = np.array([trip[i][0] for i in perm]), np.array([trip[i][1] for i in perm])
    vals = np.array([trip[i][2] for i in perm], dtype=dt)
    shape = (2, 20)
    for coo in (False, True):
        p, j, x = _run(shape, rows, cols, vals, SUM, coo)
        assert p.tolist() == [0, 8, 12]
        assert np.array_equal(_bits(x[:8]), _bits(np.array(singles, dtype=dt)))   # single entries: bit for bit
        row1 = dict(zip(j[8:].tolist(), x[8:]))
        assert np.isnan(row1[4].real) and (not cx or row1[4].imag == 2.0)
        assert row1[2] == 0 and not np.signbit(row1[2].real)                      # kept as +0.0
        assert np.signbit(row1[6].real) and row1[6] == 0
        p, j, x = _run(shape, rows, cols, vals, SUM | DROP, coo)
        # dropped: -0.0, (0, -0.0), (0, 0) for a real type, and the sums that cancelled or stayed -0.0
        zero_singles = [k for k, v in enumerate(singles) if v == 0]
        assert len(zero_singles) == (2 if cx else 3)
        assert j[:p[1]].tolist() == [2 * k + 1 for k in range(8) if k not in zero_singles]
        assert j[p[1]:].tolist() == [4, 9]
    p, j, x = _run(shape, rows, cols, vals, DROP, False)
    keep = vals != 0
    assert x.size == keep.sum() and np.isnan(x.view(rd)).any() and (np.abs(x.view(rd)) == den).any()


# ------------------------------------------------------------------ 6. determinism
def test_same_call_twice_gives_identical_bytes():
    shape, rows, cols, vals = _runs_across(np.complex128, seed=1000)
    for ops, coo in [(SUM, False), (SUM | DROP, True), (SORT, True)]:
        a = _run(shape, rows, cols, vals, ops, coo, check=False)
        b = _run(shape, rows, cols, vals, ops, coo, check=False)
        assert all(np.array_equal(_bits(u), _bits(v)) for u, v in zip(a, b))


# ------------------------------------------------------------------ 7. status codes
def test_status_codes():
    shape, rows, cols, vals = _mixed_input(np.float64, seed=1100)
    c = _Call(shape, rows, cols, vals, SUM, False)
    c.h.set_timing(True)
    try:
        assert c.query() == 0 and c.need.value > 0
        assert sum(n for _, n in c.h.get_timing().values()) == 0          # a size query launches nothing
    finally:
        c.h.set_timing(False)
    assert c.structure(shrink=1) == INVALID_VALUE                         # a workspace that is too small
    assert c.structure() == 0 and c.values() == 0
    sv.assert_same_special(c.result(), c.reference())
    z = _Call(shape, rows, cols, vals, 0, False)                          # CSR with nothing to do
    assert z.query() == INVALID_VALUE
    bad = _Call(shape, rows, cols, vals, 8, True)                         # an unknown op bit
    assert bad.query() == INVALID_VALUE


@pytest.mark.parametrize("m,n", [(0, 0), (0, 7), (7, 0), (7, 5)])
def test_degenerate_shapes(m, n):
    e = np.zeros(0, dtype=np.int64)
    for ops in OPS:
        for coo in _forms(ops):
            c = _Call((m, n), e, e, np.zeros(0), ops, coo)
            assert c.query() == 0 and c.structure() == 0 and c.nnz.value == 0
            assert c.values() == 0
            torch.cuda.synchronize()
            p = c.cp_t.cpu().numpy()
            assert not p[:m + 1].any() and (_bits(p[m + 1:]) == 0xFF).all()


# ------------------------------------------------------------------ 8. the Python layer
def _dev_csr(shape, p, j, x, device):
    from spmm_amd.sparse import csr_matrix
    return csr_matrix((torch.from_numpy(x.copy()), torch.from_numpy(j.copy()), torch.from_numpy(p.copy())),
                      shape=shape, device=device, canonical=False)


def _dev_coo(shape, rows, cols, vals, device):
    from spmm_amd.sparse import coo_matrix
    return coo_matrix((torch.from_numpy(vals.copy()), (torch.from_numpy(rows.copy()), torch.from_numpy(cols.copy()))),
                      shape=shape, device=device)


def _same_tensors(a, b):
    assert len(a) == len(b)
    for u, v in zip(a, b):
        assert u.dtype == v.dtype and u.shape == v.shape
        assert np.array_equal(_bits(u.cpu().numpy()), _bits(v.cpu().numpy()))


@pytest.mark.parametrize("name", list(DTYPES))
def test_containers_equal_their_torch_paths(name):
    """Each call on GPU tensors gives byte for byte what it gives on CPU copies (the torch path)."""
    dt = DTYPES[name]
    m, n = 80, 400
    rows, cols, vals = cc.pool_triplets(m, n, 6000, 2500, dt, seed=1200)
    vals[::6] = 0
    p, j, x = cc.as_csr(m, rows, cols, vals)
    for method in ("sum_duplicates", "eliminate_zeros"):
        g, c = _dev_csr((m, n), p, j, x, DEV), _dev_csr((m, n), p, j, x, "cpu")
        getattr(g, method)()
        getattr(c, method)()
        assert g.data.is_cuda and g.nnz < vals.size
        _same_tensors((g.indptr, g.indices, g.data), (c.indptr, c.indices, c.data))
        assert g._canonical == c._canonical
    g, c = _dev_coo((m, n), rows, cols, vals, DEV).tocsr(), _dev_coo((m, n), rows, cols, vals, "cpu").tocsr()
    _same_tensors((g.indptr, g.indices, g.data), (c.indptr, c.indices, c.data))
    assert g.has_canonical_format
    for method in ("sum_duplicates", "eliminate_zeros"):
        g, c = _dev_coo((m, n), rows, cols, vals, DEV), _dev_coo((m, n), rows, cols, vals, "cpu")
        getattr(g, method)()
        getattr(c, method)()
        assert g.nnz < vals.size
        _same_tensors((g.row, g.col, g.data), (c.row, c.col, c.data))


@pytest.mark.parametrize("name", list(DTYPES))
def test_containers_equal_scipy_where_it_is_determinate(name):
    dt = DTYPES[name]
    m, n = 120, 300
    rows, cols, vals = cc.mult2_triplets(m, n, 5000, 0.5, dt, seed=1300)
    vals[::8] = 0
    p, j, x = cc.as_csr(m, rows, cols, vals)
    S = cc.scipy_csr((m, n), p, j, x)
    S.sum_duplicates()
    g = _dev_csr((m, n), p, j, x, DEV)
    g.sum_duplicates()
    G = g.get()
    sv.assert_same_special((G.indptr, G.indices, G.data), (S.indptr, S.indices, S.data))
    G = _dev_coo((m, n), rows, cols, vals, DEV).tocsr().get()
    sv.assert_same_special((G.indptr, G.indices, G.data), (S.indptr, S.indices, S.data))
    Z = cc.scipy_csr((m, n), p, j, x)
    Z.eliminate_zeros()
    g = _dev_csr((m, n), p, j, x, DEV)
    g.eliminate_zeros()
    G = g.get()
    sv.assert_same_special((G.indptr, G.indices, G.data), (Z.indptr, Z.indices, Z.data))


def test_cusparse_canonicalize_and_csrsort():
    from spmm_amd import cusparse
    m, n = 80, 400
    rows, cols, vals = cc.pool_triplets(m, n, 6000, 2500, np.float64, seed=1400)
    vals[::6] = 0
    p, j, x = cc.as_csr(m, rows, cols, vals)
    r = cc.rows_of(p)
    flags = [(True, True, False, SUM), (True, True, True, SUM | DROP), (True, False, False, SORT),
             (False, False, True, DROP), (True, False, True, SORT | DROP)]
    for sort, sm, ez, ops in flags:
        g = _dev_csr((m, n), p, j, x, DEV)
        out = cusparse.canonicalize(g, sort=sort, sum_duplicates=sm, eliminate_zeros=ez)
        assert out is not g and g.nnz == vals.size                             # a new matrix
        sv.assert_same_special((out.indptr.cpu().numpy(), out.indices.cpu().numpy(), out.data.cpu().numpy()),
                               cc.restate((m, n), r, j, x, ops))
        assert (out._canonical is True) == sm
        out = cusparse.canonicalize(_dev_coo((m, n), rows, cols, vals, DEV), sort=sort, sum_duplicates=sm,
                                    eliminate_zeros=ez)
        sv.assert_same_special((out.indptr.cpu().numpy(), out.indices.cpu().numpy(), out.data.cpu().numpy()),
                               cc.restate((m, n), rows, cols, vals, ops, coo=True))
    out = cusparse.canonicalize(_dev_coo((m, n), rows, cols, vals, DEV), sort=False, sum_duplicates=False)
    sv.assert_same_special((out.indptr.cpu().numpy(), out.indices.cpu().numpy(), out.data.cpu().numpy()),
                           cc.restate((m, n), rows, cols, vals, 0, coo=True))
    g = _dev_csr((m, n), p, j, x, DEV)
    before = g.indptr
    assert cusparse.csrsort(g) is None                                         # in place, duplicates kept
    assert g.indptr is before and g.nnz == vals.size
    sv.assert_same_special((g.indptr.cpu().numpy(), g.indices.cpu().numpy(), g.data.cpu().numpy()),
                           cc.restate((m, n), r, j, x, SORT))
    with pytest.raises(RuntimeError):
        cusparse.canonicalize(_dev_csr((m, n), p, j, x, "cpu"))
    with pytest.raises(TypeError):
        cusparse.csrsort(_dev_coo((m, n), rows, cols, vals, DEV))


# ------------------------------------------------------------------ 9. operators
def test_operators_on_non_canonical_operands(monkeypatch):
    """A @ B, A + B and A.T @ A of operands with unsorted rows and duplicates (multiplicity <= 2, so
    scipy's own sums are determinate) equal scipy, and they get there through spg_canonicalize."""
    from spmm_amd import cusparse
    calls = []
    real = cusparse._canonicalize_arrays

    def counted(*a, **k):
        calls.append(a[5])
        return real(*a, **k)
    monkeypatch.setattr(cusparse, "_canonicalize_arrays", counted)
    m = n = 300
    ta = cc.mult2_triplets(m, n, 3000, 0.5, np.float64, seed=1500)
    tb = cc.mult2_triplets(m, n, 3000, 0.5, np.float64, seed=1501)
    pa, pb = cc.as_csr(m, *ta), cc.as_csr(m, *tb)
    SA, SB = cc.scipy_csr((m, n), *pa), cc.scipy_csr((m, n), *pb)
    SA.sum_duplicates()
    SB.sum_duplicates()

    def dev():
        return _dev_csr((m, n), *pa, DEV), _dev_csr((m, n), *pb, DEV)

    def same(G, S, drop=False):
        G, S = G.get(), sp.csr_matrix(S)
        S.sort_indices()
        if drop:
            G.eliminate_zeros()
            S.eliminate_zeros()
        sv.assert_same_special((G.indptr, G.indices, G.data), (S.indptr, S.indices, S.data))
    A, B = dev()
    same(A @ B, SA @ SB)
    assert calls == [SUM, SUM]
    A, B = dev()
    same(A + B, SA + SB, drop=True)
    assert calls == [SUM] * 4
    A, _ = dev()
    same(A.T @ A, SA.T.tocsr() @ SA)
    assert len(calls) >= 6 and set(calls) == {SUM}
