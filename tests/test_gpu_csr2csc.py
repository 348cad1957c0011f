"""Device CSR transpose (spg_csr2csc; cupyx.cusparse.csr2csc / csc2csr, modify_src/cupy-src/
cupyx/cusparse.py:1014-1035, :1092-1113) and the transposed products that inherit it.

Bar: AT's indptr, indices and the BYTES of its values equal scipy's ``tocsc()`` -- a stable
counting sort, duplicates and unsorted rows kept in stored order -- for the four value types and
both row-pointer types; values are moved bit for bit (NaN sign and payload included); transposed
products equal scipy's bit for bit.

The kernel's seams (spmm_amd/csrc/spgemm_transpose.hpp): a wave walks its chunk 64 entries at a
time (WAVE), one wave owns TR_CHUNK = 2048 entries, a workgroup TR_WPB * TR_CHUNK = 8192
(TR_BLOCK_ENTRIES); the number of 8-bit digit passes changes at 256, 65536 and 2**24 columns.
"""
import ctypes
import functools

import numpy as np
import pytest
import scipy.sparse as sp

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64, np.complex64, np.complex128]
IPS = [np.int32, np.int64]
WAVE, TR_CHUNK, TR_BLOCK_ENTRIES = 64, 2048, 8192
M, K = 600, 500
HOT, EMPTY_COLS = 7, (0, 250, K - 1)
INVALID_VALUE = 3


def _bits(v):
    return np.ascontiguousarray(v).view(np.uint8)


def _values(rng, shape, dt):
    v = rng.standard_normal(shape)
    if np.dtype(dt).kind == "c":
        v = v + 1j * rng.standard_normal(shape)
    return v.astype(dt)


def _same(got, want):
    """got: (indptr, indices, data) from the device; want: scipy's csc (or csr) matrix."""
    p, j, x = got
    assert np.array_equal(p.astype(np.int64), want.indptr.astype(np.int64)), "indptr"
    assert np.array_equal(j, want.indices), "indices"
    assert x.dtype == want.data.dtype
    assert np.array_equal(_bits(x), _bits(want.data)), "value bytes"


def _parts(m):
    torch.cuda.synchronize()
    return m.indptr.cpu().numpy(), m.indices.cpu().numpy(), m.data.cpu().numpy()


def _raw(S, ip=np.int32, fill=None, shrink=0, mutate=None, timing=False):
    """spg_csr2csc through ctypes on the scipy CSR S (taken as stored: nothing canonicalised).
    fill: byte the workspace and the three output arrays hold before the call; shrink: bytes
    taken off the queried workspace size; mutate(vt): edits AT's descriptor before the call.
    Returns (status, (indptr, indices, data) | None, queried bytes, timing | None)."""
    from spmm_amd import _lib
    from spmm_amd.cusparse import _IT, _VT
    dev = "cuda:0"
    h = _lib.get_handle(0)
    h.set_stream(torch.cuda.current_stream(0).cuda_stream)
    m, n = S.shape
    tip = torch.int32 if ip == np.int32 else torch.int64
    ap = torch.from_numpy(S.indptr.astype(ip)).to(dev)
    aj = torch.from_numpy(S.indices.astype(np.int32)).to(dev)
    ax = torch.from_numpy(S.data.copy()).to(dev)
    nnz = int(S.indptr[-1])

    def buf(count, dtype):
        t = torch.empty(max(count, 1), dtype=dtype, device=dev)
        if fill is not None:
            t.view(torch.uint8).fill_(fill)
        return t
    tp, tj, tx = buf(n + 1, tip), buf(nnz, torch.int32), buf(nnz, ax.dtype)
    va = _lib.SpgCsr(m, n, nnz, ap.data_ptr(), aj.data_ptr() if nnz else 0, ax.data_ptr() if nnz else 0,
                     _IT[tip], _VT[ax.dtype])
    vt = _lib.SpgCsr(n, m, nnz, tp.data_ptr(), tj.data_ptr() if nnz else 0, tx.data_ptr() if nnz else 0,
                     _IT[tip], _VT[ax.dtype])
    if mutate is not None:
        mutate(vt)
    if timing:
        h.set_timing(True)
    try:
        need = ctypes.c_size_t(0)
        st = h.lib.spg_csr2csc(h.ptr, ctypes.byref(va), ctypes.byref(vt), ctypes.byref(need), None)
        if st != 0:
            return st, None, 0, None
        after_query = h.get_timing() if timing else None
        ws = buf(need.value, torch.uint8)
        have = ctypes.c_size_t(need.value - shrink)
        st = h.lib.spg_csr2csc(h.ptr, ctypes.byref(va), ctypes.byref(vt), ctypes.byref(have),
                               ctypes.c_void_p(ws.data_ptr()))
        torch.cuda.synchronize()
        t = (after_query, h.get_timing()) if timing else None
    finally:
        if timing:
            h.set_timing(False)
    if st != 0:
        return st, None, need.value, t
    return 0, (tp[:n + 1].cpu().numpy(), tj[:nnz].cpu().numpy(), tx[:nnz].cpu().numpy()), need.value, t


# ------------------------------------------------------------------ 1. edge matrix
@functools.lru_cache(maxsize=None)
def _edge_matrix(dt):
    """600 x 500 canonical CSR: rows of 0, 1, 63, 64, 65 and 200 entries, a run of empty rows,
    otherwise a random fill; column HOT is hit by every non-empty row; columns 0, 250 and 499
    are empty."""
    rng = np.random.default_rng(11)
    lens = rng.integers(0, 40, size=M)
    lens[:6] = [0, 1, 63, 64, 65, 200]
    lens[100:171] = 0
    lens[M - 1] = 130
    free = np.setdiff1d(np.arange(K), np.array(EMPTY_COLS + (HOT,)))
    rows = []
    for n in lens:
        rows.append(np.sort(np.append(rng.choice(free, size=int(n) - 1, replace=False), HOT)) if n else
                    np.zeros(0, dtype=np.int64))
    indptr = np.zeros(M + 1, dtype=np.int32)
    indptr[1:] = np.cumsum(lens)
    indices = np.concatenate(rows).astype(np.int32)
    A = sp.csr_matrix((_values(rng, indices.size, dt), indices, indptr), shape=(M, K))
    assert A.has_canonical_format
    cnt = np.bincount(A.indices, minlength=K)
    assert all(cnt[c] == 0 for c in EMPTY_COLS) and cnt[HOT] == np.count_nonzero(lens)
    return A


@functools.lru_cache(maxsize=None)
def _edge_device(dt):
    from spmm_amd.sparse import csr_matrix
    return csr_matrix(_edge_matrix(dt), device="cuda:0")


@pytest.mark.parametrize("ip", IPS)
@pytest.mark.parametrize("dt", DTYPES)
def test_edge_matrix(dt, ip):
    S = _edge_matrix(dt)
    st, got, _, _ = _raw(S, ip)
    assert st == 0
    assert got[0].dtype == ip
    _same(got, S.tocsc())


# ------------------------------------------------------------------ 2. entry-count seams
COUNTS = [0, 1, WAVE - 1, WAVE, WAVE + 1, TR_CHUNK - 1, TR_CHUNK, TR_CHUNK + 1,
          TR_BLOCK_ENTRIES - 1, TR_BLOCK_ENTRIES, TR_BLOCK_ENTRIES + 1, 3 * TR_BLOCK_ENTRIES + 5]


@functools.lru_cache(maxsize=None)
def _seam_matrix(kind, nnz):
    rng = np.random.default_rng(1000 + nnz)
    data = rng.standard_normal(nnz)
    if kind == "row":       # 1 x n: one row holds every entry
        n = nnz + 3
        return sp.csr_matrix((data, np.sort(rng.choice(n, size=nnz, replace=False)).astype(np.int32),
                              np.array([0, nnz], dtype=np.int32)), shape=(1, n))
    if kind == "col":       # n x 1: every entry in column 0
        n = nnz + 3
        has = np.zeros(n, dtype=np.int64)
        has[rng.choice(n, size=nnz, replace=False)] = 1
        indptr = np.zeros(n + 1, dtype=np.int32)
        indptr[1:] = np.cumsum(has)
        return sp.csr_matrix((data, np.zeros(nnz, dtype=np.int32), indptr), shape=(n, 1))
    cells = np.sort(rng.choice(300 * 257, size=nnz, replace=False))   # random 300 x 257
    indptr = np.zeros(301, dtype=np.int32)
    indptr[1:] = np.cumsum(np.bincount(cells // 257, minlength=300))
    return sp.csr_matrix((data, (cells % 257).astype(np.int32), indptr), shape=(300, 257))


@pytest.mark.parametrize("ip", IPS)
@pytest.mark.parametrize("nnz", COUNTS)
@pytest.mark.parametrize("kind", ["row", "col", "random"])
def test_entry_count_seams(kind, nnz, ip):
    """nnz around the batch of 64 (WAVE), the wave chunk (TR_CHUNK = 2048), the workgroup
    (TR_BLOCK_ENTRIES = 8192), and one size over three workgroups."""
    S = _seam_matrix(kind, nnz)
    assert S.nnz == nnz
    st, got, _, _ = _raw(S, ip)
    assert st == 0
    _same(got, S.tocsc())


# ------------------------------------------------------------------ 3. width seams
@functools.lru_cache(maxsize=None)
def _width_matrix(cols):
    rows = 64
    rng = np.random.default_rng(cols % 9973)
    nnz = min(5000, rows * cols)
    cells = rng.choice(rows * cols, size=nnz, replace=False)
    cells = np.unique(np.concatenate([cells, [0, cols - 1, (rows - 1) * cols, rows * cols - 1]]))
    indptr = np.zeros(rows + 1, dtype=np.int32)
    indptr[1:] = np.cumsum(np.bincount(cells // cols, minlength=rows))
    S = sp.csr_matrix((rng.standard_normal(cells.size), (cells % cols).astype(np.int32), indptr),
                      shape=(rows, cols))
    assert S.indices.min() == 0 and S.indices.max() == cols - 1
    return S


@pytest.mark.parametrize("ip", IPS)
@pytest.mark.parametrize("cols", [1, 255, 256, 257, 65535, 65536, 65537, 2 ** 24 + 3])
def test_width_seams(cols, ip):
    """One more digit pass from 257, 65537 and 2**24 + 1 columns on; entries in the first and
    the last column."""
    S = _width_matrix(cols)
    st, got, _, _ = _raw(S, ip)
    assert st == 0
    _same(got, S.tocsc())


@pytest.mark.parametrize("ip", IPS)
@pytest.mark.parametrize("shape", [(0, 5), (5, 0), (0, 0), (1, 1)])
def test_empty_and_tiny(shape, ip):
    S = sp.csr_matrix(shape, dtype=np.float64)
    st, got, _, _ = _raw(S, ip, fill=0xFF)
    assert st == 0
    _same(got, S.tocsc())
    if shape == (1, 1):
        S = sp.csr_matrix(np.array([[2.5]]))
        st, got, _, _ = _raw(S, ip, fill=0xFF)
        assert st == 0
        _same(got, S.tocsc())


# ------------------------------------------------------------------ 4. non-canonical input
@pytest.mark.parametrize("ip", IPS)
def test_noncanonical_literal(ip):
    """Unsorted rows and duplicates stay, in stored order (scipy's csr_tocsc)."""
    S = sp.csr_matrix((np.arange(1.0, 10.0), np.array([3, 1, 3, 0, 2, 2, 1, 3, 1], dtype=np.int32),
                       np.array([0, 4, 6, 6, 9], dtype=np.int32)), shape=(4, 5))
    st, (p, j, x), _, _ = _raw(S, ip)
    assert st == 0
    assert p.tolist() == [0, 1, 4, 6, 9, 9]
    assert j.tolist() == [0, 0, 3, 3, 1, 1, 0, 0, 3]
    assert x.tolist() == [4, 2, 7, 9, 5, 6, 1, 3, 8]


@functools.lru_cache(maxsize=None)
def _shuffled_matrix(dt):
    """200 x 90, every row's entries shuffled, about 10 % of the entries stored twice."""
    rng = np.random.default_rng(77)
    B = sp.random(200, 90, density=0.2, format="csr", random_state=rng)
    r = np.repeat(np.arange(200), np.diff(B.indptr))
    c = B.indices
    dup = rng.choice(r.size, size=r.size // 10, replace=False)
    r, c = np.concatenate([r, r[dup]]), np.concatenate([c, c[dup]])
    order = np.lexsort((rng.random(r.size), r))   # rows ascending, random inside a row
    indptr = np.zeros(201, dtype=np.int32)
    indptr[1:] = np.cumsum(np.bincount(r, minlength=200))
    S = sp.csr_matrix((_values(rng, r.size, dt), c[order].astype(np.int32), indptr), shape=(200, 90))
    assert not S.has_canonical_format and not S.has_sorted_indices
    return S


@pytest.mark.parametrize("ip", IPS)
@pytest.mark.parametrize("dt", DTYPES)
def test_noncanonical_random(dt, ip):
    from spmm_amd import cusparse
    from spmm_amd.sparse import csr_matrix
    S = _shuffled_matrix(dt)
    st, got, _, _ = _raw(S, ip)
    assert st == 0
    _same(got, S.tocsc())
    if ip == np.int32:   # the Python entry point keeps the duplicates too
        T = cusparse.csr2csc(csr_matrix((S.data, S.indices, S.indptr), shape=S.shape, device="cuda:0"))
        assert T.shape == S.shape and T._canonical is None
        _same(_parts(T), S.tocsc())


@pytest.mark.parametrize("dt", DTYPES)
def test_noncanonical_containers_still_canonicalise(dt):
    """transpose_csr() and csc.tocsr() keep their contract -- a canonical CSR result -- for
    non-canonical input: the engine's stable transpose, then duplicates summed.  No cell is
    stored more than twice here, so the sums do not depend on an order."""
    from spmm_amd.sparse import csc_matrix, csr_matrix
    S = _shuffled_matrix(dt)
    want = S.T.tocsr()
    want.sum_duplicates()
    A = csr_matrix((S.data, S.indices, S.indptr), shape=S.shape, device="cuda:0")
    C = csc_matrix((S.data, S.indices, S.indptr), shape=S.shape[::-1], device="cuda:0")   # S^T in CSC
    for got in (A.transpose_csr(), C.tocsr()):
        assert got.shape == want.shape and got._canonical is True
        _same(_parts(got), want)


# ------------------------------------------------------------------ 5. special values
def _special_components(rdt, n, rng):
    """n components of the real type rdt drawn from: quiet and signalling NaNs with distinct
    payloads and both signs, +-0, the smallest denormal (both signs), +-inf, and normals."""
    if rdt == np.float32:
        u, pool = np.uint32, [0x7FC00001, 0xFFC00123, 0x7F800001, 0xFF800ABC, 0x7FFFFFFF, 0x00000000, 0x80000000,
                              0x00000001, 0x80000001, 0x7F800000, 0xFF800000, 0x3F800000, 0xC0490FDB]
    else:
        u, pool = np.uint64, [0x7FF8000000000001, 0xFFF8000000000123, 0x7FF0000000000001, 0xFFF0000000000ABC,
                              0x7FFFFFFFFFFFFFFF, 0x0000000000000000, 0x8000000000000000, 0x0000000000000001,
                              0x8000000000000001, 0x7FF0000000000000, 0xFFF0000000000000, 0x3FF0000000000000,
                              0xC00921FB54442D18]
    pool = np.array(pool, dtype=u)
    picks = np.concatenate([pool, pool[rng.integers(0, pool.size, size=n)]])[:n]
    return rng.permutation(picks)


@pytest.mark.parametrize("ip", IPS)
@pytest.mark.parametrize("dt", DTYPES)
def test_special_values_move_bit_for_bit(dt, ip):
    """Output bytes = input bytes under scipy's permutation (taken from a copy of the matrix whose
    values are the entry numbers, so the host never computes on a NaN)."""
    S = _edge_matrix(dt)
    rng = np.random.default_rng(5)
    rdt = np.float32 if dt in (np.float32, np.complex64) else np.float64
    ncomp = 2 if np.dtype(dt).kind == "c" else 1
    comps = _special_components(rdt, S.nnz * ncomp, rng)   # both halves of a complex
    data = comps.view(rdt).view(dt) if ncomp == 2 else comps.view(dt)
    assert data.size == S.nnz
    tags = sp.csr_matrix((np.arange(S.nnz, dtype=np.float64), S.indices, S.indptr), shape=S.shape).tocsc()
    perm = tags.data.astype(np.int64)
    src = sp.csr_matrix((data, S.indices, S.indptr), shape=S.shape)
    st, (p, j, x), _, _ = _raw(src, ip)
    assert st == 0
    assert np.array_equal(p.astype(np.int64), tags.indptr) and np.array_equal(j, tags.indices)
    item = np.dtype(dt).itemsize
    want = _bits(data).reshape(-1, item)[perm]
    assert np.array_equal(_bits(x).reshape(-1, item), want)


# ------------------------------------------------------------------ 6. round trip
@pytest.mark.parametrize("dt", DTYPES)
def test_round_trip_and_canonical_flag(dt):
    from spmm_amd import _lib, cusparse
    S = _edge_matrix(dt)
    A = _edge_device(dt)
    h = _lib.get_handle(0)
    h.set_timing(True)
    try:
        C = cusparse.csr2csc(A)
        back = cusparse.csc2csr(C)
        t1, t2, t3 = A.tocsc(), A.T.tocsr(), A.transpose_csr()
        validates = h.get_timing()["validate"][1]
    finally:
        h.set_timing(False)
    assert validates == 0
    assert C._canonical is True and back._canonical is True
    assert t1._canonical is True and t2._canonical is True and t3._canonical is True
    assert C.shape == S.shape and back.shape == S.shape
    _same(_parts(C), S.tocsc())
    _same(_parts(back), S)
    want = S.T.tocsr()
    assert t2.shape == want.shape and t3.shape == want.shape and t1.shape == S.shape
    for t in (t1, t2, t3):
        _same(_parts(t), want)
    assert A.T.data.data_ptr() == A.data.data_ptr() and A.T.shape == (K, M)


# ------------------------------------------------------------------ 7. products
@functools.lru_cache(maxsize=None)
def _dense(dt, rows, n):
    X = _values(np.random.default_rng(300 + rows + n), (rows, n), dt)
    X.setflags(write=False)
    return X


def _host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


@pytest.mark.parametrize("dt", DTYPES)
def test_spmv_transa_bitexact(dt):
    from spmm_amd import cusparse
    S = _edge_matrix(dt)
    x = _dense(dt, M, 1)[:, 0]
    got = _host(cusparse.spmv(_edge_device(dt), torch.from_numpy(x.copy()).cuda(), transa=True))
    want = S.T @ x
    assert got.dtype == want.dtype and np.array_equal(_bits(got), _bits(want))


@pytest.mark.parametrize("n", [1, 17, 130])
@pytest.mark.parametrize("dt", DTYPES)
def test_spmm_transa_bitexact(dt, n):
    from spmm_amd import cusparse
    S = _edge_matrix(dt)
    X = _dense(dt, M, n)
    got = _host(cusparse.spmm(_edge_device(dt), torch.from_numpy(X.copy()).cuda(), transa=True))
    want = S.T @ X
    assert got.shape == want.shape and got.dtype == want.dtype
    assert np.array_equal(_bits(got), _bits(want))


@pytest.mark.parametrize("n", [1, 17, 130])
@pytest.mark.parametrize("dt", DTYPES)
def test_csc_operand_bitexact(dt, n):
    from spmm_amd.sparse import csc_matrix
    S = _edge_matrix(dt)
    X = _dense(dt, K, n)
    got = _host(csc_matrix(S, "cuda:0") @ torch.from_numpy(X.copy()).cuda())
    want = S.tocsc() @ X
    assert got.shape == want.shape and got.dtype == want.dtype
    assert np.array_equal(_bits(got), _bits(want))


@pytest.mark.parametrize("dt", DTYPES)
def test_AT_A_bitexact(dt):
    """A.T @ A with A.T the csc view: sorted columns, exact zeros dropped, as the SpGEMM parity
    tests compare."""
    S = _edge_matrix(dt)
    A = _edge_device(dt)
    C = A.T @ A
    p, j, x = _parts(C)
    got = sp.csr_matrix((x, j, p), shape=C.shape)
    got.eliminate_zeros()
    want = (S.T @ S).tocsr()
    want.sort_indices()
    want.eliminate_zeros()
    assert got.shape == want.shape == (K, K)
    _same((got.indptr, got.indices, got.data), want)


# ------------------------------------------------------------------ 8. workspace and statuses
def test_size_query_launches_nothing_and_call_is_timed():
    from spmm_amd import _lib
    S = _edge_matrix(np.float64)
    st, got, need, (after_query, after_call) = _raw(S, timing=True)
    assert st == 0 and need > 0
    assert all(launches == 0 for _, launches in after_query.values())
    assert after_call["b_layout"][1] > 0 and after_call["scan"][1] > 0
    assert after_call["validate"][1] == 0
    assert len(_lib.PHASES) == 9 and len(after_call) == 9
    _same(got, S.tocsc())


def test_workspace_too_small_is_invalid_value():
    st, got, need, _ = _raw(_edge_matrix(np.float64), shrink=1)
    assert st == INVALID_VALUE and got is None and need > 0


@pytest.mark.parametrize("what", ["rows", "cols", "nnz", "value_type", "indptr_type", "indptr", "indices"])
def test_mismatched_descriptor_is_invalid_value(what):
    from spmm_amd import _lib

    def mutate(vt):
        if what in ("rows", "cols", "nnz"):
            setattr(vt, what, getattr(vt, what) + 1)
        elif what == "value_type":
            vt.value_type = _lib.SPG_R_32F
        elif what == "indptr_type":
            vt.indptr_type = _lib.SPG_INDEX_64I
        else:
            setattr(vt, what, None)
    st, got, _, _ = _raw(_edge_matrix(np.float64), mutate=mutate)
    assert st == INVALID_VALUE and got is None


def test_null_arguments_are_invalid_value():
    from spmm_amd import _lib
    h = _lib.get_handle(0)
    v = _lib.SpgCsr()
    need = ctypes.c_size_t(0)
    assert h.lib.spg_csr2csc(h.ptr, None, ctypes.byref(v), ctypes.byref(need), None) == INVALID_VALUE
    assert h.lib.spg_csr2csc(h.ptr, ctypes.byref(v), None, ctypes.byref(need), None) == INVALID_VALUE
    assert h.lib.spg_csr2csc(h.ptr, ctypes.byref(v), ctypes.byref(v), None, None) == INVALID_VALUE


# ------------------------------------------------------------------ 9. poisoned buffers
@pytest.mark.parametrize("ip", IPS)
@pytest.mark.parametrize("name", ["edge", "wide", "shuffled"])
def test_poisoned_buffers(name, ip):
    """The same result with the workspace and the outputs pre-filled with 0xFF and with 0x00:
    nothing stale is read, nothing relies on zeroed memory (two, three and one digit passes)."""
    S = {"edge": lambda: _edge_matrix(np.complex128), "wide": lambda: _width_matrix(65537),
         "shuffled": lambda: _shuffled_matrix(np.float32)}[name]()
    want = S.tocsc()
    for fill in (0xFF, 0x00):
        st, got, _, _ = _raw(S, ip, fill=fill)
        assert st == 0
        _same(got, want)
