"""Device submatrix extraction (spg_csr_extract_nnz / spg_csr_extract; cupyx's __getitem__,
modify_src/cupy-src/cupyx/scipy/sparse/_index.py:348) through the C ABI, and the containers'
``A[rows, cols]`` that runs on it.

Bar (tests/index_cases.py): the row pointer, the indices and the bits of the values equal
index_cases.restate -- the rule of include/spgemm.h in numpy, itself held to scipy by
tests/test_index_cpu.py -- array for array, for the four value types, both row-pointer types of A
and both of C.  Every output and the workspace are tests.guarded buffers poisoned 0xFF, their
guard bands checked after the calls.

The kernels' seams (spmm_amd/csrc/spgemm_extract.hpp): k_ex_fill walks a chunk of EX_CHUNK = 1024
output entries 64 at a time, a workgroup holds EX_WPB = 4 waves (4096 entries); a step whose 64
outputs lie in one output row searches a window of S bounded once; the scans work in tiles of
SCAN_TILE = 2048; the column list is sorted in chunks of TR_CHUNK = 2048 positions.

Not tested here: SPG_STATUS_OVERFLOW and source positions past 2**31 (tests/test_gpu_index_large.py).
"""
import ctypes
import functools

import numpy as np
import pytest
import scipy.sparse as sp

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import index_cases as ic          # noqa: E402
from tests.guarded import guarded            # noqa: E402

IPCP = [(np.int32, np.int32), (np.int32, np.int64), (np.int64, np.int32), (np.int64, np.int64)]
NOT_INITIALIZED, INVALID_VALUE, NOT_SUPPORTED = 1, 3, 10
DEV = "cuda:0"


def _ipcp_id(v):
    return "A%d-C%d" % (np.dtype(v[0]).itemsize * 8, np.dtype(v[1]).itemsize * 8)


def _name(dt):
    return np.dtype(dt).name


class _Operand:
    """A scipy CSR matrix on the device with an `ip` row pointer, and its descriptor."""

    def __init__(self, S, ip=np.int32):
        from spmm_amd import _lib
        from spmm_amd.cusparse import _IT, _VT
        self.S, self.shape = S, S.shape
        self.p = torch.from_numpy(S.indptr.astype(ip)).to(DEV)
        self.j = torch.from_numpy(S.indices.astype(np.int32)).to(DEV)
        self.x = torch.from_numpy(S.data.copy()).to(DEV)
        nnz = int(S.indptr[-1])
        self.view = _lib.SpgCsr(S.shape[0], S.shape[1], nnz, self.p.data_ptr(), self.j.data_ptr() if nnz else 0,
                                self.x.data_ptr() if nnz else 0, _IT[self.p.dtype], _VT[self.x.dtype])


@functools.lru_cache(maxsize=8)
def _operand(which, dt, ip):
    make = {"seam": ic.seam_matrix, "duplicates": ic.duplicate_matrix, **ic.MATRICES}[which]
    return _Operand(make(dt), ip)


class _Call:
    """One extraction through ctypes, step by step.  fill: the byte the workspace and the three
    output arrays hold before the calls."""

    def __init__(self, A, rs, cs, cp=np.int32, fill=0xFF):
        from spmm_amd import _lib
        from spmm_amd.cusparse import _IT, _VT
        self.lib_mod, self._VT = _lib, _VT
        self.h = _lib.get_handle(0)
        self.h.set_stream(torch.cuda.current_stream(0).cuda_stream)
        self.lib, self.fill, self.A = self.h.lib, fill, A
        self.tcp = torch.int32 if cp == np.int32 else torch.int64
        self.ctype = _IT[self.tcp]
        self.keep = []
        self.rows, self.cols = self.sel(rs), self.sel(cs)
        self.nr, self.nc = ic.count_of(rs, A.shape[0]), ic.count_of(cs, A.shape[1])
        self.cp_t = guarded(self.nr + 1, self.tcp, fill, DEV, "C_indptr")
        self.nnz = ctypes.c_int64(-1)
        self.need = ctypes.c_size_t(0)
        self.ws = self.vc = self.cj = self.cx = None

    def sel(self, s):
        if s is None:
            return None
        if s[0] == "range":
            v = self.lib_mod.SpgSel(s[1], s[2], s[3], None)
        else:
            t = torch.tensor(list(s[1]) or [0], dtype=torch.int32, device=DEV)
            self.keep.append(t)
            v = self.lib_mod.SpgSel(0, 0, len(s[1]), t.data_ptr())
        self.keep.append(v)
        return ctypes.byref(v)

    def query(self):
        return self.lib.spg_csr_extract_nnz(self.h.ptr, ctypes.byref(self.A.view), self.rows, self.cols, None,
                                            self.ctype, ctypes.byref(self.nnz), ctypes.byref(self.need), None)

    def structure(self, shrink=0):
        self.ws = guarded(self.need.value, torch.uint8, self.fill, DEV, "workspace")
        have = ctypes.c_size_t(self.need.value - shrink)
        return self.lib.spg_csr_extract_nnz(self.h.ptr, ctypes.byref(self.A.view), self.rows, self.cols,
                                            ctypes.c_void_p(self.cp_t.data_ptr()), self.ctype, ctypes.byref(self.nnz),
                                            ctypes.byref(have), ctypes.c_void_p(self.ws.data_ptr()))

    def alloc_c(self):
        n = int(self.nnz.value)
        self.cj = guarded(n, torch.int32, self.fill, DEV, "C_indices")
        self.cx = guarded(n, self.A.x.dtype, self.fill, DEV, "C_values")
        self.vc = self.lib_mod.SpgCsr(self.nr, self.nc, n, self.cp_t.data_ptr(), self.cj.data_ptr() if n else 0,
                                      self.cx.data_ptr() if n else 0, self.ctype, self._VT[self.A.x.dtype])

    def values(self, shrink=0):
        if self.vc is None:
            self.alloc_c()
        return self.lib.spg_csr_extract(self.h.ptr, ctypes.byref(self.A.view), self.rows, self.cols,
                                        ctypes.byref(self.vc), ctypes.c_size_t(self.need.value - shrink),
                                        ctypes.c_void_p(self.ws.data_ptr()))

    def result(self):
        torch.cuda.synchronize()
        for g in (self.cp_t, self.ws, self.cj, self.cx):
            g.check()
        return self.cp_t.t.cpu().numpy(), self.cj.t.cpu().numpy(), self.cx.t.cpu().numpy()


def _run(A, rs, cs, cp=np.int32, fill=0xFF):
    c = _Call(A, rs, cs, cp, fill)
    assert c.query() == 0 and c.need.value > 0
    assert c.structure() == 0
    assert c.values() == 0
    got = c.result()
    assert got[0].dtype == cp and int(got[0][-1]) == c.nnz.value == got[1].size
    return got


@functools.lru_cache(maxsize=None)
def _want(which, dt, cid):
    """index_cases.restate of one case, computed once and never written."""
    if which == "seam":
        rs, cs = {c[0]: c[1:] for c in ic.seam_cases()}[cid]
        return ic.expected(ic.seam_matrix(dt), rs, cs)
    rs, cs = {c[0]: c[2:] for c in ic.cases()}[cid]
    return ic.expected(ic.MATRICES[which](dt), rs, cs)


# ------------------------------------------------------------------ 1. the shared case list
@pytest.mark.parametrize("ipcp", IPCP, ids=_ipcp_id)
@pytest.mark.parametrize("dt", ic.DTYPES, ids=_name)
@pytest.mark.parametrize("name", list(ic.MATRICES))
def test_case_list(name, dt, ipcp):
    A = _operand(name, dt, ipcp[0])
    for cid, cname, rs, cs in ic.cases():
        if cname == name:
            ic.same_arrays(_want(name, dt, cid), _run(A, rs, cs, ipcp[1]), cid)


# ------------------------------------------------------------------ 2. the kernels' seams
@pytest.mark.parametrize("ipcp", IPCP, ids=_ipcp_id)
@pytest.mark.parametrize("dt", ic.DTYPES, ids=_name)
def test_seams(dt, ipcp):
    """Row lengths on each side of a wave, a chunk and a workgroup; output rows that start and end
    mid-step; a long row three times; a reversed permutation; one source entry feeding three fill
    steps (a column listed 130 times); a list that selects nothing present; a column step of -3;
    K = all over a span that starts at an odd entry."""
    A = _operand("seam", dt, ipcp[0])
    assert int(A.S.indptr[16]) == 1
    for cid, rs, cs in ic.seam_cases():
        ic.same_arrays(_want("seam", dt, cid), _run(A, rs, cs, ipcp[1]), cid)


@pytest.mark.parametrize("ipcp", IPCP, ids=_ipcp_id)
@pytest.mark.parametrize("dt", [np.float32, np.complex128], ids=_name)
def test_duplicates_under_a_repeated_column_list(dt, ipcp):
    """A non-canonical A with duplicate (row, column) entries: every stored duplicate gives every
    repeat of its column, in stored order and ascending list position."""
    S = ic.duplicate_matrix(dt)
    A = _operand("duplicates", dt, ipcp[0])
    rng = np.random.default_rng(5)
    cols = ("list", [int(v) for v in rng.integers(0, 64, 300)])
    for rs in (None, ("list", [int(v) for v in rng.integers(0, 40, 90)]), ("range", 39, -2, 20)):
        ic.same_arrays(ic.expected(S, rs, cols), _run(A, rs, cols, ipcp[1]))


@pytest.mark.parametrize("k", [2047, 2048, 2049, 4097])
def test_column_list_sort_seams(k):
    """The list's sort at one and two chunks of TR_CHUNK = 2048 positions; 5000 columns take two
    digit passes."""
    S = ic.seam_matrix(np.float64)
    A = _operand("seam", np.float64, np.int32)
    rng = np.random.default_rng(k)
    cols = ("list", [int(v) for v in rng.integers(0, 5000, k)])
    rows = ("list", [ic.SEAM_LONG, 63, 55])
    ic.same_arrays(ic.expected(S, rows, cols), _run(A, rows, cols))


@functools.lru_cache(maxsize=None)
def _pass_count_case(width):
    """A of 40 rows and about 600 entries over `width` columns, a list of 300 positions with
    repeats (four in five of them columns A holds), and index_cases.expected of A[:, list]."""
    rng = np.random.default_rng(width)
    rows = [np.sort(rng.choice(width, int(n), replace=False)) for n in rng.integers(0, 31, 40)]
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    indices = np.concatenate(rows).astype(np.int32)
    S = sp.csr_matrix((rng.standard_normal(indices.size), indices, indptr), shape=(40, width))
    held = rng.choice(indices, 60)
    picks = np.where(rng.random(300) < 0.8, rng.choice(held, 300), rng.integers(0, width, 300))
    cols = ("list", [int(v) for v in picks])
    assert len(set(cols[1])) < 300 and max(cols[1]) >= (width - 1) // 2
    return S, cols, ic.expected(S, None, cols)


@pytest.mark.parametrize("ipcp", [IPCP[0], IPCP[3]], ids=_ipcp_id)
@pytest.mark.parametrize("width,passes", [(200, 1), (70000, 3), ((1 << 24) + 3, 4)])
def test_column_list_sort_pass_counts(width, passes, ipcp):
    """The list's sort over one, three and four digit passes (the bytes of width - 1): the sorted
    records end in one ping-pong buffer or the other by the parity of the pass count."""
    assert (max(width - 1, 1).bit_length() + 7) // 8 == passes
    S, cols, want = _pass_count_case(width)
    assert want[1].size >= 200
    ic.same_arrays(want, _run(_Operand(S, ipcp[0]), None, cols, ipcp[1]), f"{passes} passes")


@pytest.mark.parametrize("nr", [2047, 2048, 2049])
def test_row_scan_seams(nr):
    """The scan over the output rows at one tile and one row past it."""
    S = ic.small(np.float64)
    A = _operand("small", np.float64, np.int32)
    rows = ("list", [int(v) for v in np.random.default_rng(nr).integers(0, 23, nr)])
    ic.same_arrays(ic.expected(S, rows, ("range", 36, -1, 30)), _run(A, rows, ("range", 36, -1, 30)))


# ------------------------------------------------------------------ 3. degenerate sizes
@pytest.mark.parametrize("ipcp", IPCP, ids=_ipcp_id)
def test_degenerate_sizes(ipcp):
    A = _operand("small", np.float64, ipcp[0])
    m, n = A.shape
    for rs, cs in ((("range", 0, 1, 0), None), (("list", []), ("list", [3, 3])), (None, ("range", 5, 1, 0)),
                   (("list", [1, 1]), ("list", [])), (("range", 0, 0, 0), ("range", 0, 0, 0))):
        p, j, x = _run(A, rs, cs, ipcp[1])
        assert p.tolist() == [0] * (ic.count_of(rs, m) + 1) and j.size == 0 and x.size == 0
    Z = _Operand(sp.csr_matrix((9, 7), dtype=np.float32), ipcp[0])
    for rs, cs in ((None, None), (("list", [8, 0, 8]), ("list", [6, 6, 1])), (("range", 8, -1, 9), ("range", 1, 2, 3))):
        p, j, x = _run(Z, rs, cs, ipcp[1])
        assert p.tolist() == [0] * (ic.count_of(rs, 9) + 1) and j.size == 0 and x.size == 0
    E = _Operand(sp.csr_matrix((0, 0), dtype=np.float64), ipcp[0])
    assert _run(E, None, None, ipcp[1])[0].tolist() == [0]
    one = _Operand(sp.csr_matrix(np.array([[2.5]])), ipcp[0])
    p, j, x = _run(one, ("list", [0, 0]), ("list", [0, 0, 0]), ipcp[1])
    assert p.tolist() == [0, 3, 6] and j.tolist() == [0, 1, 2] * 2 and x.tolist() == [2.5] * 6
    p, j, x = _run(one, ("range", 0, 0, 1), ("range", 0, 0, 1), ipcp[1])      # step 0 with one member
    assert p.tolist() == [0, 1] and j.tolist() == [0] and x.tolist() == [2.5]


# ------------------------------------------------------------------ 4. poisoned buffers, two runs
@pytest.mark.parametrize("ipcp", IPCP, ids=_ipcp_id)
@pytest.mark.parametrize("cid", ["column_130_times_between_others", "rows_step_2_cols_step_minus_3",
                                 "reversed_permutation", "odd_span_all_cols"])
def test_identical_from_run_to_run(cid, ipcp):
    """The same bytes with the workspace and the outputs pre-filled with 0xFF and with 0x00, and
    from one run to the next: nothing stale is read, nothing relies on zeroed memory."""
    dt = np.float32
    A = _operand("seam", dt, ipcp[0])
    rs, cs = {c[0]: c[1:] for c in ic.seam_cases()}[cid]
    runs = [_run(A, rs, cs, ipcp[1], fill=f) for f in (0xFF, 0x00, 0xFF, 0x00)]
    ic.same_arrays(_want("seam", dt, cid), runs[0], cid)
    for r in runs[1:]:
        for a, b in zip(r, runs[0]):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ------------------------------------------------------------------ 5. statuses, workspace, timing
def _small_call(rs=("list", [5, 0, 5]), cs=("range", 2, 3, 10)):
    return _Call(_operand("small", np.float64, np.int32), rs, cs)


@pytest.mark.parametrize("kind", ["all", "range", "list"])
def test_size_query_launches_nothing_and_phases(kind):
    from spmm_amd import _lib
    S = ic.seam_matrix(np.float64)
    cs = {"all": None, "range": ("range", 4999, -3, 1000), "list": ("list", [17] * 130 + list(range(0, 5000, 7)))}[kind]
    rs = ("list", [ic.SEAM_LONG, 55, ic.SEAM_LONG])
    c = _Call(_operand("seam", np.float64, np.int32), rs, cs)
    c.h.set_timing(True)
    try:
        assert c.query() == 0 and c.need.value > 0
        after_query = c.h.get_timing()
        assert c.structure() == 0
        after_nnz = c.h.get_timing()
        assert c.values() == 0
        torch.cuda.synchronize()
        after = c.h.get_timing()
    finally:
        c.h.set_timing(False)
    assert all(n == 0 for _, n in after_query.values())
    passes = 2                                              # 5000 columns: 13 bits, two 8-bit digits
    want = {"all": dict(symbolic=1, scan=1, b_layout=0), "range": dict(symbolic=2, scan=2, b_layout=0),
            "list": dict(symbolic=2, scan=2 + passes, b_layout=2 + 2 * passes)}[kind]
    assert {k: after_nnz[k][1] for k in want} == want and after_nnz["numeric"][1] == 0
    assert after["numeric"][1] == 1
    assert all(n == 0 for k, (_, n) in after.items() if k not in ("symbolic", "scan", "numeric", "b_layout"))
    assert len(_lib.PHASES) == 9 and len(after) == 9
    ic.same_arrays(ic.expected(S, rs, cs), c.result())


def test_workspace_one_byte_short():
    c = _small_call()
    assert c.query() == 0
    assert c.structure(shrink=1) == INVALID_VALUE
    assert c.structure() == 0
    assert c.values(shrink=1) == INVALID_VALUE
    assert c.values() == 0
    ic.same_arrays(ic.expected(ic.small(), ("list", [5, 0, 5]), ("range", 2, 3, 10)), c.result())


def test_null_arguments():
    c = _small_call()
    lib, h = c.lib, c.h.ptr
    a, nnz, need = ctypes.byref(c.A.view), ctypes.byref(c.nnz), ctypes.byref(c.need)
    r, k = c.rows, c.cols
    assert lib.spg_csr_extract_nnz(None, a, r, k, None, c.ctype, nnz, need, None) == NOT_INITIALIZED
    assert lib.spg_csr_extract_nnz(None, None, r, k, None, c.ctype, None, None, None) == NOT_INITIALIZED
    assert lib.spg_csr_extract_nnz(h, None, r, k, None, c.ctype, nnz, need, None) == INVALID_VALUE
    assert lib.spg_csr_extract_nnz(h, a, r, k, None, c.ctype, None, need, None) == INVALID_VALUE
    assert lib.spg_csr_extract_nnz(h, a, r, k, None, c.ctype, nnz, None, None) == INVALID_VALUE
    assert lib.spg_csr_extract_nnz(h, a, r, k, None, 16, nnz, need, None) == INVALID_VALUE       # bad C_indptr_type
    assert c.query() == 0
    ws = guarded(c.need.value, torch.uint8, 0xFF, DEV)
    wsp = ctypes.c_void_p(ws.data_ptr())
    assert lib.spg_csr_extract_nnz(h, a, r, k, None, c.ctype, nnz, need, wsp) == INVALID_VALUE   # NULL C_indptr with a workspace
    assert c.structure() == 0
    c.alloc_c()
    vc, n, wsp = ctypes.byref(c.vc), ctypes.c_size_t(c.need.value), ctypes.c_void_p(c.ws.data_ptr())
    assert lib.spg_csr_extract(None, a, r, k, vc, n, wsp) == NOT_INITIALIZED
    assert lib.spg_csr_extract(h, None, r, k, vc, n, wsp) == INVALID_VALUE
    assert lib.spg_csr_extract(h, a, r, k, None, n, wsp) == INVALID_VALUE
    assert lib.spg_csr_extract(h, a, r, k, vc, n, None) == INVALID_VALUE
    assert lib.spg_csr_extract(h, a, r, k, vc, n, wsp) == 0
    ic.same_arrays(ic.expected(ic.small(), ("list", [5, 0, 5]), ("range", 2, 3, 10)), c.result())


BAD_RANGES = [("range", 0, 1, -1), ("range", 0, 0, 2), ("range", -1, 1, 3), ("range", 23, 1, 1), ("range", 20, 1, 4),
              ("range", 3, -2, 3), ("range", 22, 1, 2), ("range", 0, -1, 2)]


@pytest.mark.parametrize("bad", BAD_RANGES, ids=lambda b: "s%d_t%d_n%d" % b[1:])
@pytest.mark.parametrize("axis", ["rows", "cols"])
def test_bad_ranges(axis, bad):
    """count < 0; step == 0 with count > 1; a first or a last member outside [0, extent) -- over
    the 23 rows, and the same numbers over the first 23 of the 37 columns moved to their end."""
    if axis == "cols":
        bad = ("range", bad[1] + (14 if bad[1] >= 20 else 0), bad[2], bad[3])
    c = _small_call(*((bad, None) if axis == "rows" else (None, bad)))
    assert c.query() == INVALID_VALUE


def test_good_range_edges():
    for rs in (("range", 22, 1, 1), ("range", 0, 5, 1), ("range", 22, -11, 3), ("range", 0, 11, 3), ("range", 7, 0, 1),
               ("range", 0, 0, 0)):
        c = _small_call(rs, None)
        assert c.query() == 0 and c.structure() == 0 and c.values() == 0
        ic.same_arrays(ic.expected(ic.small(), rs, None), c.result())


def test_not_supported_extents():
    from spmm_amd import _lib
    c = _small_call()
    big = _lib.SpgSel(0, 1, 2 ** 31, c.keep[0].data_ptr())     # a list of 2**31 entries (never read)
    lib, h = c.lib, c.h.ptr
    a, nnz, need = ctypes.byref(c.A.view), ctypes.byref(c.nnz), ctypes.byref(c.need)
    assert lib.spg_csr_extract_nnz(h, a, ctypes.byref(big), None, None, c.ctype, nnz, need, None) == NOT_SUPPORTED
    assert lib.spg_csr_extract_nnz(h, a, None, ctypes.byref(big), None, c.ctype, nnz, need, None) == NOT_SUPPORTED
    wide = _lib.SpgCsr(23, 2 ** 31, c.A.view.nnz, c.A.p.data_ptr(), c.A.j.data_ptr(), c.A.x.data_ptr(),
                       c.A.view.indptr_type, c.A.view.value_type)
    assert lib.spg_csr_extract_nnz(h, ctypes.byref(wide), None, None, None, c.ctype, nnz, need, None) == NOT_SUPPORTED
    most = _lib.SpgSel(0, 1, 2 ** 31 - 1, c.keep[0].data_ptr())
    assert lib.spg_csr_extract_nnz(h, a, ctypes.byref(most), None, None, c.ctype, nnz, need, None) == 0


@pytest.mark.parametrize("what", ["indptr", "indices", "values", "indptr_type", "value_type", "nnz"])
def test_bad_operand(what):
    from spmm_amd import _lib
    c = _small_call()
    v = c.A.view
    bad = _lib.SpgCsr(v.rows, v.cols, v.nnz, v.indptr, v.indices, v.values, v.indptr_type, v.value_type)
    setattr(bad, what, {"indptr_type": 16, "nnz": -1, "value_type": 77}.get(what, None))
    status = c.lib.spg_csr_extract_nnz(c.h.ptr, ctypes.byref(bad), c.rows, c.cols, None, c.ctype, ctypes.byref(c.nnz),
                                       ctypes.byref(c.need), None)
    assert status == (NOT_SUPPORTED if what == "value_type" else INVALID_VALUE)   # (an unknown value type, as check_csr answers it)


@pytest.mark.parametrize("what", ["rows", "cols", "value_type", "indptr_type", "indptr", "indices", "values", "nnz"])
def test_mismatched_result(what):
    """C against the selections: nr x nc and A's value type; a row-pointer type that is no index
    type; NULL arrays; a negative entry count."""
    from spmm_amd import _lib
    c = _small_call()
    assert c.query() == 0 and c.structure() == 0
    c.alloc_c()
    assert c.vc.nnz > 0
    if what in ("rows", "cols"):
        setattr(c.vc, what, getattr(c.vc, what) + 1)
    elif what == "value_type":
        c.vc.value_type = _lib.SPG_R_32F
    elif what == "indptr_type":
        c.vc.indptr_type = 16
    elif what == "nnz":
        c.vc.nnz = -1
    else:
        setattr(c.vc, what, None)
    assert c.values() == INVALID_VALUE


# ------------------------------------------------------------------ 6. the Python layer
def _parts(m):
    torch.cuda.synchronize()
    return m.indptr.cpu().numpy(), m.indices.cpu().numpy(), m.data.cpu().numpy()


def _dev(S):
    from spmm_amd.sparse import csr_matrix
    return csr_matrix(S, device=DEV)


@pytest.mark.parametrize("dt", ic.DTYPES, ids=_name)
def test_getitem_runs_on_the_engine(dt):
    from spmm_amd import _lib, cusparse
    from spmm_amd.sparse import csc_matrix, csr_matrix
    S = ic.small(dt)
    A = _dev(S)
    m, n = S.shape
    h = _lib.get_handle(0)
    h.set_timing(True)
    try:
        C1, C2 = A[[5, 0, 5], 2:32:3], A[::-1][:, [3, 3, 36, 0]]
        torch.cuda.synchronize()
        launches = h.get_timing()
    finally:
        h.set_timing(False)
    assert launches["numeric"][1] == 3                      # the engine ran, not torch
    assert isinstance(C1, csr_matrix) and C1.indptr.dtype == torch.int32 and C1.device.type == "cuda"
    ic.same_arrays(ic.expected(S, ("list", [5, 0, 5]), ("range", 2, 3, 10)), _parts(C1))
    ic.same_arrays(ic.expected(S, ("range", m - 1, -1, m), ("list", [3, 3, 36, 0])), _parts(C2))
    assert C1._canonical is True and C2._canonical is None and C2.has_canonical_format is False
    for cid, cname, rs, cs in ic.cases()[::5]:
        if cname == "small":
            ic.same_arrays(_want("small", dt, cid), _parts(A[ic.py_key(rs, m)][:, ic.py_key(cs, n)]), cid)
    E = cusparse.extract(A, rows=[5, 0, 5], cols=[36, 1, 36])       # one selection per axis, also for two lists
    ic.same_arrays(ic.expected(S, ("list", [5, 0, 5]), ("list", [36, 1, 36])), _parts(E))
    ic.same_arrays(ic.expected(S, None, ("range", 30, -2, 10)), _parts(cusparse.extract(A, cols=slice(30, 10, -2))))
    T = csc_matrix((A.data, A.indices, A.indptr), shape=(n, m))     # the arrays read as A^T in CSC
    G = T[torch.tensor([36, 1, 36], device=DEV), 20:2:-3]
    assert isinstance(G, csc_matrix) and G.shape == (3, 6)
    ic.same_arrays(ic.expected(S, ("range", 20, -3, 6), ("list", [36, 1, 36])), _parts(G))
    assert isinstance(cusparse.extract(T, rows=[0]), csc_matrix)
    D = S.toarray()
    assert A[7, 36] == D[7, 36] and A[-1, -1] == D[-1, -1] and A[4, 0] == 0
    with pytest.raises(IndexError):
        A[[0, m]]
    with pytest.raises(IndexError):
        A[:, torch.tensor([-n - 1], device=DEV)]
    with pytest.raises(NotImplementedError):
        A[[0, 1], [0, 1]]
    with pytest.raises(TypeError, match="unsupported type"):
        cusparse.extract(S)
    with pytest.raises(RuntimeError, match="device-resident"):
        cusparse.extract(csr_matrix(S, device="cpu"))


def test_sampled_rows_of_a_product():
    """(A[rows] @ B) equals (A @ B)[rows] array for array: N = 1024, density 0.01, 97 random rows."""
    from tests.golden_cases import load
    A, B, _, _ = load("config1_n1024_d0.01_f64")
    assert A.shape == (1024, 1024)
    rows = np.random.default_rng(97).choice(1024, 97, replace=False)
    dA, dB = _dev(A), _dev(B)
    left, right = dA[rows] @ dB, (dA @ dB)[rows]
    assert left.shape == right.shape == (97, 1024) and left.nnz > 0
    ic.same_arrays(_parts(right), _parts(left))
    R = (A @ B)[rows]
    R.sort_indices()
    assert np.array_equal(R.indptr, _parts(left)[0]) and np.array_equal(R.indices, _parts(left)[1])
