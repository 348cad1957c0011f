"""Device dense <-> CSR conversion (spg_csr2dense, spg_dense2csr_nnz + spg_dense2csr; cupyx's
csr2dense / dense2csr, modify_src/cupy-src/cupyx/cusparse.py:768-829, :1146-1228, and the kernels
behind toarray() and csr_matrix(dense), cupyx/scipy/sparse/_csr.py:383-428, :1158-1210).

Bar, csr2dense: equal to scipy's ``toarray()`` by tests/special_values.py's rule (every component
that is not NaN bit for bit, NaN exactly where scipy has one) for the four value types, both
row-pointer types and both orders; every element of the extent written, the bytes between the minor
extent and ld and both guard bands untouched; the same bytes from run to run.
Bar, dense2csr: indptr, indices and the BYTES of the values equal scipy's ``csr_matrix(D)`` (NaN
sign and payload included); both orders, any ld.

The kernels' seams (spmm_amd/csrc/spgemm_dense.hpp): a wave walks a row 64 entries at a time (WAVE);
csr2dense's workgroup owns R = 8 rows x W = 512 columns; dense2csr cuts rows into segments of
S = 1024 columns and reads a column-major D in tiles of T = 64 rows; row-major operands take
16-byte accesses when the base and ld * sizeof are multiples of 16.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import dense_cases as dc        # noqa: E402
from tests import special_values as sv     # noqa: E402
from tests.guarded import guarded          # noqa: E402

WAVE, W, R, S, T = 64, 512, 8, 1024, 64     # mirrors of spgemm_dense.hpp (checked below)
assert (WAVE, W, R, S, T) == (dc.WAVE, dc.W, dc.R, dc.S, dc.T)
DNAMES = list(dc.DTYPES)
IPS = [np.int32, np.int64]
ORDERS = ["row", "col"]
INVALID_VALUE = 3
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_constants_mirror_the_kernels():
    # (DV_S and DV_T size dn_layout's table too: the kernels take them from the carves' header)
    for header, names in (("spgemm_dense.hpp", (("DV_W", W), ("DV_R", R))),
                          ("spg_format_layouts.hpp", (("DV_S", S), ("DV_T", T)))):
        text = open(os.path.join(ROOT, "spmm_amd", "csrc", header)).read()
        for name, v in names:
            assert f"constexpr int {name} = {v};" in text, name
    assert '#include "spg_format_layouts.hpp"' in open(os.path.join(ROOT, "spmm_amd", "csrc", "spgemm_dense.hpp")).read()


def _handle():
    from spmm_amd import _lib
    h = _lib.get_handle(0)
    h.set_stream(torch.cuda.current_stream(0).cuda_stream)
    return h


def _tdt(dt):
    return getattr(torch, np.dtype(dt).name)


def _order(order):
    from spmm_amd import _lib
    return _lib.SPG_ORDER_ROW if order == "row" else _lib.SPG_ORDER_COL


# ------------------------------------------------------------------ raw calls
def raw_todense(A, ip=np.int32, order="row", pad=0, offset=0, fill=0xFF, mutate=None, timing=False):
    """spg_csr2dense through ctypes on the scipy CSR A (taken as stored) into a guarded buffer of
    `offset` + major * ld elements, ld = minor extent + pad, D starting `offset` elements in.
    Checks the guard bands and that every byte outside the extent still holds `fill`.
    Returns (status, m x n array | None, timing | None)."""
    from spmm_amd import _lib
    from spmm_amd.cusparse import _IT, _VT
    h = _handle()
    m, n = A.shape
    dt = A.dtype
    tip = torch.int32 if ip == np.int32 else torch.int64
    nnz = int(A.indptr[-1])
    ap = torch.from_numpy(A.indptr.astype(ip)).to(DEV)
    aj = torch.from_numpy(A.indices.astype(np.int32)).to(DEV)
    ax = torch.from_numpy(A.data.copy()).to(DEV)
    major, minor = (m, n) if order == "row" else (n, m)
    ld = minor + pad
    g = guarded(offset + major * ld, dt, fill, DEV, "D")
    item = np.dtype(dt).itemsize
    va = _lib.SpgCsr(m, n, nnz, ap.data_ptr(), aj.data_ptr() if nnz else 0, ax.data_ptr() if nnz else 0,
                     _IT[tip], _VT[_tdt(dt)])
    vd = _lib.SpgDense(m, n, ld, g.data_ptr() + offset * item, _order(order), _VT[_tdt(dt)])
    if mutate is not None:
        mutate(va, vd)
    if timing:
        h.set_timing(True)
    try:
        st = h.lib.spg_csr2dense(h.ptr, ctypes.byref(va), ctypes.byref(vd))
        torch.cuda.synchronize()
        t = h.get_timing() if timing else None
    finally:
        if timing:
            h.set_timing(False)
    g.check()
    raw = g.bytes().cpu().numpy()
    if st != 0:
        assert (raw == fill).all(), "a rejected call wrote to D"
        return st, None, t
    written = np.zeros(offset + major * ld, dtype=bool)
    body = written[offset:].reshape(major, ld) if major * ld else written[offset:].reshape(major, 0)
    body[:, :minor] = True
    outside = ~np.repeat(written, item)
    assert (raw[outside] == fill).all(), "bytes outside the extent changed (ld padding or the lead-in)"
    vals = raw.view(dt)[offset:]
    got = vals.reshape(major, ld)[:, :minor] if major * ld else np.zeros((major, minor), dtype=dt)
    return 0, (got if order == "row" else got.T), t


def _upload_dense(D, order, pad, offset):
    """D in a device buffer of the given order, ld = minor + pad, starting `offset` elements in;
    the lead-in and the padding hold 1.0 (a conversion that read them would count them)."""
    m, n = D.shape
    major, minor = (m, n) if order == "row" else (n, m)
    ld = minor + pad
    host = np.ones(offset + major * ld, dtype=D.dtype)
    if major * ld:
        host[offset:].reshape(major, ld)[:, :minor] = D if order == "row" else D.T
    dev = torch.from_numpy(host).to(DEV)
    return dev, ld


def raw_fromdense(D, cp=np.int32, order="row", pad=0, offset=0, fill=0xFF, shrink=0, mutate=None, timing=False):
    """spg_dense2csr_nnz + spg_dense2csr through ctypes on the numpy array D; workspace, row
    pointer, indices and values are guarded buffers poisoned with `fill`.
    Returns (status, (indptr, indices, data) | None, nnz, queried bytes, timing | None)."""
    from spmm_amd import _lib
    from spmm_amd.cusparse import _IT, _VT
    h = _handle()
    m, n = D.shape
    dt = D.dtype
    tcp = torch.int32 if cp == np.int32 else torch.int64
    dev, ld = _upload_dense(D, order, pad, offset)
    item = np.dtype(dt).itemsize
    vd = _lib.SpgDense(m, n, ld, (dev.data_ptr() + offset * item) if dev.numel() else 0, _order(order),
                       _VT[_tdt(dt)])
    if mutate is not None:
        mutate(vd, None)
    gp = guarded(m + 1, tcp, fill, DEV, "C.indptr")
    need, nnz = ctypes.c_size_t(0), ctypes.c_int64(-1)
    t = None
    if timing:
        h.set_timing(True)
    try:
        st = h.lib.spg_dense2csr_nnz(h.ptr, ctypes.byref(vd), None, _IT[tcp], ctypes.byref(nnz), ctypes.byref(need),
                                     None)
        if st != 0:
            return st, None, None, 0, None
        after_query = h.get_timing() if timing else None
        gw = guarded(need.value, "uint8", fill, DEV, "workspace")
        have = ctypes.c_size_t(need.value - shrink)
        st = h.lib.spg_dense2csr_nnz(h.ptr, ctypes.byref(vd), ctypes.c_void_p(gp.data_ptr()), _IT[tcp],
                                     ctypes.byref(nnz), ctypes.byref(have), ctypes.c_void_p(gw.data_ptr()))
        torch.cuda.synchronize()
        gp.check(), gw.check()
        if st != 0:
            return st, None, int(nnz.value), need.value, None
        after_nnz = h.get_timing() if timing else None
        nc = int(nnz.value)
        gj, gx = guarded(nc, torch.int32, fill, DEV, "C.indices"), guarded(nc, dt, fill, DEV, "C.values")
        vc = _lib.SpgCsr(m, n, nc, gp.data_ptr(), gj.data_ptr() if nc else 0, gx.data_ptr() if nc else 0, _IT[tcp],
                         _VT[_tdt(dt)])
        if mutate is not None:
            mutate(vd, vc)
        st = h.lib.spg_dense2csr(h.ptr, ctypes.byref(vd), ctypes.byref(vc), have, ctypes.c_void_p(gw.data_ptr()))
        torch.cuda.synchronize()
        if timing:
            t = (after_query, after_nnz, h.get_timing())
    finally:
        if timing:
            h.set_timing(False)
    for g in (gp, gw, gj, gx):
        g.check()
    if st != 0:
        return st, None, nc, need.value, t
    return 0, (gp.t.cpu().numpy(), gj.t.cpu().numpy(), gx.t.cpu().numpy()), nc, need.value, t


def _same_csr(got, want, what=""):
    p, j, x = got
    assert np.array_equal(p.astype(np.int64), want.indptr.astype(np.int64)), f"{what}: indptr"
    assert np.array_equal(j, want.indices), f"{what}: indices"
    assert x.dtype == want.data.dtype
    assert np.array_equal(dc.bits(x), dc.bits(want.data)), f"{what}: value bytes"


def _toarray(A):
    with np.errstate(all="ignore"):
        return A.toarray()


# ------------------------------------------------------------------ 1. csr2dense: shapes on the seams
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("ip", IPS)
@pytest.mark.parametrize("dname", DNAMES)
def test_todense_shape_seams(dname, ip, order):
    """Row lengths 0, 1, 63, 64, 65 and full; n around 64, W and 2W; m around R and 3R; the buffer
    poisoned with 0xFF and with 0x00."""
    for m, n in dc.TODENSE_SHAPES:
        A = dc.lengths_case(dname, m, n)
        want = _toarray(A)
        for fill in (0xFF, 0x00):
            st, got, _ = raw_todense(A, ip, order, fill=fill)
            assert st == 0
            assert np.array_equal(dc.bits(got), dc.bits(want)), (m, n, fill)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("dname", DNAMES)
def test_todense_alignment_paths(dname, order):
    """n (and m) odd with ld = extent, ld = extent + 3, and a base one element past a 16-byte
    boundary (the scalar path); even extents with ld a multiple of 16 bytes (the 16-byte path)."""
    for m, n in ((R + 1, 65), (R + 1, W + 1), (R, 2 * W)):
        A = dc.lengths_case(dname, m, n)
        want = _toarray(A)
        for pad, offset in ((0, 0), (3, 0), (0, 1), (3, 1), (4, 0), (4, 4)):
            st, got, _ = raw_todense(A, np.int32, order, pad=pad, offset=offset)
            assert st == 0
            assert np.array_equal(dc.bits(got), dc.bits(want)), (m, n, pad, offset)


# ------------------------------------------------------------------ 2. csr2dense: duplicates
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("ip", IPS)
@pytest.mark.parametrize("dname", DNAMES)
def test_todense_duplicates_in_stored_order(dname, ip, order):
    A = dc.duplicates_case(dname)
    assert not A.has_canonical_format
    want = _toarray(A)
    st, got, _ = raw_todense(A, ip, order)
    assert st == 0
    for cell in dc.TRIPLE_CELLS:      # 1.0 or 2.0 here is a wrong order of addition
        assert got[cell] == 0 and not np.signbit(got[cell].real), (cell, got[cell])
    assert np.array_equal(dc.bits(got), dc.bits(want))
    assert np.array_equal(dc.bits(got), dc.bits(dc.ref_todense(A)))


# ------------------------------------------------------------------ 3. csr2dense: special values
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("dname", DNAMES)
def test_todense_special_values(dname, order):
    """+-0, denormals, +-inf and NaN as lone entries and as summands, complex values with one
    zero part; a lone -0.0 arrives as +0.0."""
    A = dc.special_case(dname)
    want = _toarray(A)
    sh = sv.classes(want)
    assert sh["nan"] > 0 and sh["inf"] > 0 and sh["denormal"] > 0
    st, got, _ = raw_todense(A, np.int32, order)
    assert st == 0
    sv.assert_values_special(np.ascontiguousarray(got), want)
    dt = dc.DTYPES[dname]
    Z = sp.csr_matrix((np.array([-0.0, -0.0, -0.0], dtype=dt), np.array([0, 2, 2], dtype=np.int32),
                       np.array([0, 3], dtype=np.int32)), shape=(1, 3))
    st, got, _ = raw_todense(Z, np.int32, order)
    assert st == 0 and not dc.bits(got).any()      # all +0.0


# ------------------------------------------------------------------ 4. csr2dense: degenerate sizes, statuses
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("ip", IPS)
def test_todense_degenerate(ip, order):
    for shape in ((0, 5), (5, 0), (0, 0), (1, 1), (R + 1, W + 1)):
        A = sp.csr_matrix(shape, dtype=np.float64)        # nnz == 0: zeros over the poison
        st, got, t = raw_todense(A, ip, order, pad=2, timing=True)
        assert st == 0 and got.shape == shape and not dc.bits(got).any()
        launches = sum(v[1] for v in t.values())
        assert launches == (0 if 0 in shape else 1)


def test_todense_statuses():
    from spmm_amd import _lib
    A = dc.lengths_case("f64", R + 1, 65)

    def run(f, **kw):
        return raw_todense(A, mutate=f, **kw)[0]
    assert run(lambda va, vd: setattr(vd, "ld", 64)) == INVALID_VALUE
    assert run(lambda va, vd: setattr(vd, "ld", R), order="col") == INVALID_VALUE
    assert run(lambda va, vd: setattr(vd, "value_type", _lib.SPG_R_32F)) == INVALID_VALUE
    assert run(lambda va, vd: setattr(vd, "rows", R)) == INVALID_VALUE
    assert run(lambda va, vd: setattr(vd, "cols", 66)) == INVALID_VALUE
    assert run(lambda va, vd: setattr(vd, "order", 0)) == INVALID_VALUE
    assert run(lambda va, vd: setattr(vd, "values", None)) == INVALID_VALUE
    assert run(lambda va, vd: setattr(va, "indices", None)) == INVALID_VALUE
    assert run(lambda va, vd: setattr(va, "indptr", None)) == INVALID_VALUE
    h = _handle()
    va, vd = _lib.SpgCsr(), _lib.SpgDense()
    assert h.lib.spg_csr2dense(h.ptr, None, ctypes.byref(vd)) == INVALID_VALUE
    assert h.lib.spg_csr2dense(h.ptr, ctypes.byref(va), None) == INVALID_VALUE
    assert h.lib.spg_csr2dense(None, ctypes.byref(va), ctypes.byref(vd)) == 1


def test_todense_is_timed_under_layout():
    A = dc.duplicates_case("f64")
    st, got, t = raw_todense(A, timing=True)
    assert st == 0 and len(t) == 9
    assert t["b_layout"][1] == 1
    assert sum(v[1] for v in t.values()) == 1


@pytest.mark.parametrize("order", ORDERS)
def test_todense_two_runs_identical(order):
    for A in (dc.duplicates_case("f32"), dc.special_case("c128")):
        a = raw_todense(A, np.int32, order)[1]
        b = raw_todense(A, np.int32, order)[1]
        assert np.array_equal(dc.bits(a), dc.bits(b))


# ------------------------------------------------------------------ 5. dense2csr: shapes on the seams
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("cp", IPS)
@pytest.mark.parametrize("dname", DNAMES)
def test_fromdense_shape_seams(dname, cp, order):
    """n around 64, S and 2S; m around R, 3R and the column-major tile T; special values (-0.0,
    0-0j, denormals, NaNs with payloads) in the first and last column of every segment."""
    for m, n in dc.FROMDENSE_SHAPES:
        D = dc.dense_case(dname, m, n)
        st, got, nnz, _, _ = raw_fromdense(D, cp, order)
        assert st == 0 and got[0].dtype == cp
        want = sp.csr_matrix(D)
        assert nnz == want.nnz
        _same_csr(got, want, f"{m}x{n}")


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("dname", DNAMES)
def test_fromdense_alignment_and_poison(dname, order):
    """Odd extents with ld = extent, + 3, a base one element past a 16-byte boundary (scalar
    loads); ld a multiple of 16 bytes (16-byte loads); poison 0xFF and 0x00 in every output and
    the workspace.  The padding holds 1.0: reading it would add entries."""
    for m, n in ((R + 1, 65), (T + 1, S + 1), (R, 2 * S)):
        D = dc.dense_case(dname, m, n)
        want = sp.csr_matrix(D)
        for pad, offset, fill in ((0, 0, 0xFF), (3, 0, 0x00), (0, 1, 0xFF), (3, 1, 0x00), (4, 0, 0xFF), (4, 4, 0x00)):
            st, got, _, _, _ = raw_fromdense(D, np.int32, order, pad=pad, offset=offset, fill=fill)
            assert st == 0
            _same_csr(got, want, f"{m}x{n} pad {pad} offset {offset}")


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("dname", DNAMES)
def test_fromdense_all_zero_and_all_nonzero(dname, order):
    for kind in ("zeros", "full"):
        D = dc.dense_case(dname, R + 1, S + 1, kind)
        st, got, nnz, _, _ = raw_fromdense(D, np.int32, order)
        assert st == 0 and nnz == (0 if kind == "zeros" else D.size)
        _same_csr(got, sp.csr_matrix(D), kind)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("cp", IPS)
def test_fromdense_degenerate(cp, order):
    for shape in ((0, 5), (5, 0), (0, 0), (1, 1)):
        D = np.zeros(shape, dtype=np.float64)
        st, got, nnz, _, t = raw_fromdense(D, cp, order, timing=True)
        assert st == 0 and nnz == 0
        _same_csr(got, sp.csr_matrix(D), str(shape))
        if 0 in shape:
            assert sum(v[1] for v in t[2].values()) == 0
    st, got, nnz, _, _ = raw_fromdense(np.array([[np.float64(5e-324)]]), cp, order)
    assert st == 0 and nnz == 1 and got[2].view(np.uint64)[0] == 1     # a denormal is kept, bit for bit


def test_fromdense_two_runs_identical():
    D = dc.dense_case("c64", T + 1, S + 1)
    for order in ORDERS:
        a = raw_fromdense(D, np.int32, order)[1]
        b = raw_fromdense(D, np.int32, order)[1]
        assert all(np.array_equal(dc.bits(x), dc.bits(y)) for x, y in zip(a, b))


# ------------------------------------------------------------------ 6. dense2csr: workspace, statuses, timing
def test_fromdense_size_query_launches_nothing_and_phases():
    D = dc.dense_case("f64", R + 1, 2 * S + 1)
    st, got, nnz, need, (after_query, after_nnz, after_fill) = raw_fromdense(D, timing=True)
    assert st == 0 and need > 0
    assert all(launches == 0 for _, launches in after_query.values())
    launches = {k: v[1] for k, v in after_nnz.items() if v[1]}
    assert launches == {"symbolic": 2, "scan": 1}          # k_dn_count + k_dn_indptr, k_scan_lb
    launches = {k: v[1] for k, v in after_fill.items() if v[1]}
    assert launches == {"symbolic": 2, "scan": 1, "numeric": 1}
    _same_csr(got, sp.csr_matrix(D))


def test_fromdense_statuses():
    from spmm_amd import _lib
    D = dc.dense_case("f64", R + 1, 65)
    st, got, _, need, _ = raw_fromdense(D, shrink=1)
    assert st == INVALID_VALUE and got is None and need > 0
    assert raw_fromdense(D, mutate=lambda vd, vc: setattr(vd, "ld", 64))[0] == INVALID_VALUE
    assert raw_fromdense(D, order="col", mutate=lambda vd, vc: setattr(vd, "ld", R))[0] == INVALID_VALUE
    assert raw_fromdense(D, mutate=lambda vd, vc: setattr(vd, "order", 7))[0] == INVALID_VALUE
    assert raw_fromdense(D, mutate=lambda vd, vc: setattr(vd, "values", None))[0] == INVALID_VALUE

    def on_c(field, value):
        return lambda vd, vc: setattr(vc, field, value) if vc is not None else None
    assert raw_fromdense(D, mutate=on_c("value_type", _lib.SPG_R_32F))[0] == INVALID_VALUE
    assert raw_fromdense(D, mutate=on_c("rows", R))[0] == INVALID_VALUE
    assert raw_fromdense(D, mutate=on_c("cols", 66))[0] == INVALID_VALUE
    assert raw_fromdense(D, mutate=on_c("indptr_type", 16))[0] == INVALID_VALUE
    assert raw_fromdense(D, mutate=on_c("indices", None))[0] == INVALID_VALUE
    assert raw_fromdense(D, mutate=on_c("indptr", None))[0] == INVALID_VALUE
    h = _handle()
    vd, vc = _lib.SpgDense(), _lib.SpgCsr()
    need, nnz = ctypes.c_size_t(0), ctypes.c_int64(0)
    f = h.lib.spg_dense2csr_nnz
    assert f(h.ptr, None, None, 32, ctypes.byref(nnz), ctypes.byref(need), None) == INVALID_VALUE
    assert f(h.ptr, ctypes.byref(vd), None, 32, None, ctypes.byref(need), None) == INVALID_VALUE
    assert f(h.ptr, ctypes.byref(vd), None, 32, ctypes.byref(nnz), None, None) == INVALID_VALUE
    ws = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    x = torch.zeros(4, dtype=torch.float64, device=DEV)
    vd = _lib.SpgDense(2, 2, 2, x.data_ptr(), _lib.SPG_ORDER_ROW, _lib.SPG_R_64F)
    assert f(h.ptr, ctypes.byref(vd), None, 32, ctypes.byref(nnz), ctypes.byref(need), None) == 0
    assert f(h.ptr, ctypes.byref(vd), None, 16, ctypes.byref(nnz), ctypes.byref(need), None) == INVALID_VALUE
    need = ctypes.c_size_t(4096)
    assert f(h.ptr, ctypes.byref(vd), None, 32, ctypes.byref(nnz), ctypes.byref(need),
             ctypes.c_void_p(ws.data_ptr())) == INVALID_VALUE          # a workspace but no C_indptr
    g = h.lib.spg_dense2csr
    assert g(h.ptr, None, ctypes.byref(vc), 4096, ctypes.c_void_p(ws.data_ptr())) == INVALID_VALUE
    assert g(h.ptr, ctypes.byref(vd), None, 4096, ctypes.c_void_p(ws.data_ptr())) == INVALID_VALUE
    assert g(h.ptr, ctypes.byref(vd), ctypes.byref(vc), 4096, None) == INVALID_VALUE


# ------------------------------------------------------------------ 7. the Python surface
def _dev_csr(A):
    from spmm_amd.sparse import csr_matrix
    return csr_matrix((A.data, A.indices, A.indptr), shape=A.shape, device=DEV)


def _host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


@pytest.mark.parametrize("dname", DNAMES)
def test_todense_method(dname):
    from spmm_amd import cusparse
    from spmm_amd.sparse import coo_matrix, csc_matrix
    A = dc.duplicates_case(dname)
    dA = _dev_csr(A)
    want = dA.get().toarray()
    d = dA.todense()
    assert isinstance(d, torch.Tensor) and d.device.type == "cuda" and d.is_contiguous()
    assert np.array_equal(dc.bits(_host(d)), dc.bits(want))
    f = dA.todense(order="F")
    assert f.stride(0) == 1 and np.array_equal(dc.bits(_host(f)), dc.bits(want))
    assert isinstance(dA.toarray(), np.ndarray) and np.array_equal(dc.bits(dA.toarray()), dc.bits(want))
    # out= views with a leading dimension, both orders; the padding keeps its contents
    m, n = A.shape
    parent = torch.full((m, n + 5), 7, dtype=d.dtype, device=DEV)
    out = parent[:, 2:2 + n]
    assert cusparse.csr2dense(dA, out=out) is out
    assert np.array_equal(dc.bits(_host(out)), dc.bits(want))
    assert bool((parent[:, :2] == 7).all()) and bool((parent[:, 2 + n:] == 7).all())
    parent = torch.full((n, m + 3), 7, dtype=d.dtype, device=DEV)
    out = parent[:, :m].t()
    assert dA.todense(out=out) is out
    assert np.array_equal(dc.bits(_host(out)), dc.bits(want)) and bool((parent[:, m:] == 7).all())
    # CSC: the same arrays read as the transpose; no transpose is made
    dC = csc_matrix((dA.data, dA.indices, dA.indptr), shape=(n, m))
    assert np.array_equal(dc.bits(_host(dC.todense())), dc.bits(want.T))
    assert np.array_equal(dc.bits(_host(cusparse.csc2dense(dC, order="F"))), dc.bits(want.T))
    assert np.array_equal(dc.bits(_host(cusparse.sparseToDense(dC))), dc.bits(want.T))
    # COO in a shuffled order
    rows = np.repeat(np.arange(m), np.diff(A.indptr))
    perm = np.random.default_rng(3).permutation(A.nnz)
    C = sp.coo_matrix((A.data[perm], (rows[perm], A.indices[perm])), shape=A.shape)
    dO = coo_matrix((torch.from_numpy(C.data).to(DEV), (C.row, C.col)), shape=A.shape, device=DEV)
    assert np.array_equal(dc.bits(_host(dO.todense())), dc.bits(C.toarray()))


@pytest.mark.parametrize("dname", DNAMES)
def test_dense_constructors(dname):
    from spmm_amd import cusparse
    from spmm_amd.sparse import csc_matrix, csr_matrix
    D = dc.dense_case(dname, T + 1, S + 1)
    t = torch.from_numpy(D.copy()).to(DEV)
    strided = torch.from_numpy(np.concatenate([D, D], axis=1)).to(DEV)[:, ::2]      # neither order: copied
    Ds = np.concatenate([D, D], axis=1)[:, ::2]
    for arg, ref in ((t, D), (t.t().contiguous().t(), D), (D, D), (strided, Ds)):
        c = csr_matrix(arg, device=DEV)
        assert c.shape == ref.shape and c._canonical is True and c.indptr.dtype == torch.int32
        assert c.device.type == "cuda" and c.has_canonical_format
        _same_csr((_host(c.indptr), _host(c.indices), _host(c.data)), sp.csr_matrix(ref))
    for c in (csc_matrix(t), cusparse.dense2csc(t), cusparse.denseToSparse(t, format="csc")):
        assert c.shape == D.shape and c.format == "csc"
        _same_csr((_host(c.indptr), _host(c.indices), _host(c.data)), sp.csc_matrix(D))
    c = cusparse.denseToSparse(t, format="coo")
    want = sp.csr_matrix(D).tocoo()
    assert np.array_equal(_host(c.row), want.row) and np.array_equal(_host(c.col), want.col)
    assert np.array_equal(dc.bits(_host(c.data)), dc.bits(want.data))


@pytest.mark.parametrize("dname", DNAMES)
def test_round_trip(dname):
    from spmm_amd.sparse import csr_matrix
    A = dc.lengths_case(dname, 3 * R + 1, W + 1).copy()
    A.data[::7] = 0                                   # explicit zeros: dropped on the way back
    dA = _dev_csr(A)
    back = csr_matrix(dA.todense())
    dA.eliminate_zeros()
    for a, b in ((back.indptr, dA.indptr), (back.indices, dA.indices)):
        assert np.array_equal(_host(a).astype(np.int64), _host(b).astype(np.int64))
    assert np.array_equal(dc.bits(_host(back.data)), dc.bits(_host(dA.data)))


def test_spmm_output_feeds_a_product():
    """spmm's dense result goes through dense2csr into ``@`` without leaving the device."""
    from spmm_amd import cusparse
    rng = np.random.default_rng(9)
    A = sp.random(200, 150, density=0.05, format="csr", random_state=rng)
    X = np.where(rng.random((150, 40)) < 0.2, rng.standard_normal((150, 40)), 0.0)
    dA = _dev_csr(A)
    Y = cusparse.spmm(dA, torch.from_numpy(X).to(DEV))
    assert np.array_equal(dc.bits(_host(Y)), dc.bits(A @ X))
    Ys = cusparse.dense2csr(Y)
    _same_csr((_host(Ys.indptr), _host(Ys.indices), _host(Ys.data)), sp.csr_matrix(A @ X))
    C = dA.T.tocsr() @ Ys
    want = (A.T.tocsr() @ sp.csr_matrix(A @ X)).tocsr()
    want.sort_indices()
    got = sp.csr_matrix((_host(C.data), _host(C.indices), _host(C.indptr)), shape=C.shape)
    got.eliminate_zeros(), want.eliminate_zeros()
    _same_csr((got.indptr, got.indices, got.data), want)


def test_python_errors():
    from spmm_amd import cusparse
    from spmm_amd.sparse import csc_matrix, csr_matrix
    A = dc.lengths_case("f64", R + 1, 65)
    dA = _dev_csr(A)
    m, n = A.shape
    with pytest.raises(TypeError):
        cusparse.csr2dense(dA.T)                      # a csc_matrix
    with pytest.raises(TypeError):
        cusparse.csc2dense(dA)
    with pytest.raises(TypeError):
        cusparse.sparseToDense(torch.zeros(2, 2, device=DEV))
    with pytest.raises(TypeError):
        cusparse.dense2csr(np.zeros((2, 2)))
    with pytest.raises(TypeError):
        cusparse.dense2csr(torch.zeros((2, 2), dtype=torch.int32, device=DEV))
    with pytest.raises(TypeError):
        dA.todense(out=torch.zeros((m, n), dtype=torch.float32, device=DEV))
    with pytest.raises(TypeError):
        cusparse.denseToSparse(torch.zeros(2, 2, device=DEV, dtype=torch.float64), format="bsr")
    with pytest.raises(ValueError):
        cusparse.dense2csr(torch.zeros(4, device=DEV, dtype=torch.float64))
    with pytest.raises(ValueError):
        dA.todense(out=torch.zeros((m, n + 1), dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError):
        dA.todense(out=torch.zeros((m, 2 * n), dtype=torch.float64, device=DEV)[:, ::2])
    with pytest.raises(ValueError):
        dA.todense(order="K")
    with pytest.raises(ValueError):
        csr_matrix(torch.zeros(3, device=DEV))
    with pytest.raises(RuntimeError):
        cusparse.dense2csr(torch.zeros(2, 2, dtype=torch.float64))
    with pytest.raises(RuntimeError):
        cusparse.csr2dense(csr_matrix((A.data, A.indices, A.indptr), shape=A.shape, device="cpu"))
    with pytest.raises(TypeError):
        csc_matrix(3.5)


def test_profiler_runs():
    """harness/dense_convert/profiler.py once at n = 512: both directions, both sides."""
    env = dict(os.environ, RUNS="2", WARMUP="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "harness", "dense_convert", "profiler.py"), "--n", "512",
                        "--densities", "0.01", "--dtypes", "float64"], capture_output=True, text=True, env=env,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "csr2dense  (a) engine wall" in r.stdout and "index_put_" in r.stdout
    assert "dense2csr  (a) engine wall" in r.stdout and "nonzero + gather" in r.stdout
    assert r.stdout.count("RESULT ") == 1 and "GB/s" in r.stdout
