"""spg_spmv and spg_spmm at their structural seams, through the C ABI, on poisoned and guarded
operands (tests/dense_seams.py, tests/guarded.py).

k_spmv / k_spmm_col: the 728-row seam matrix (a wave's 64 rows on each side of the LDS chunk: an
entry total of ch - 1, ch, ch + 1 and 2 * ch, an empty row on the chunk boundary, a row that
straddles it, rows of three chunks and more at lane 0, 31 and 63, an empty group, a ragged last
group) and, for k_spmv, matrices of 1, 63, 64, 65, 255, 256 and 257 rows (the ragged wave and the
waves of a block that leave at once).  k_spmm_row / k_spmm_row_packed: 71 rows whose lengths sit
on each side of the 64-entry batch and of the 8- and 4-entry unrolls, at every packed lane-group
width with scalar and with 16-byte accesses, and at the first width past the packed kernel.

Every case: all four value types, both row-pointer widths, (alpha, beta) in {(1, 0), (a, 0),
(1, b), (a, b)}.  The output is a guarded buffer: with beta == 0 it starts as NaN (so a row that is
never stored -- an empty row, whose value is alpha * 0 -- shows), with beta != 0 as
standard_normal; the leading-dimension padding holds the poison and must keep it; x / B are
guarded too and must come back byte for byte.  The reference is oracle.spmv / oracle.spmm (equal
to scipy's products on these inputs, tests/test_dense_seams_cpu.py) followed by
special_values.axpby, the separately rounded host restatement of the epilogue.  Bit for bit.
"""
import ctypes

import numpy as np
import pytest

from oracle import oracle
from tests import dense_seams as ds
from tests import instantiations as inst
from tests import special_values as sv
from tests.guarded import guarded

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DNAMES = list(inst.DTYPES)
FILL_OF = {32: 0xFF, 64: 0x00}     # both poisons, one per row-pointer width


def _bits(v):
    return np.ascontiguousarray(v).view(np.uint8)


def _handle():
    from spmm_amd import _lib
    h = _lib.get_handle(0)
    h.set_stream(torch.cuda.current_stream().cuda_stream)
    return h


def _scalar(dname, v):
    ct = ctypes.c_float if dname in ("f32", "c64") else ctypes.c_double
    if dname.startswith("c"):
        return (ct * 2)(complex(v).real, complex(v).imag)
    return ct(float(v))


def _pairs(dname):
    a, b = inst.alpha_of(dname), ds.beta_of(dname)
    return [(1.0, 0.0), (a, 0.0), (1.0, b), (a, b)]


def _nan(dname):
    return complex(float("nan"), float("nan")) if dname.startswith("c") else float("nan")


def _upload(g, host):
    g.copy_(torch.from_numpy(np.array(host, order="C")).to(DEV))     # (a writable copy)


def _padding_intact(t, fill, what):
    if t.numel():
        assert bool((t.contiguous().view(torch.uint8) == fill).all()), f"{what}: leading-dimension padding written"


def _spmv_case(A, dname, what):
    from spmm_amd import _lib
    dt = inst.DTYPES[dname]
    m, k = A.shape
    h = _handle()
    dA = inst.Uploaded(A, DEV)
    x = ds.dense_values("x", (k,), dt)
    y0 = ds.dense_values("y0", (m,), dt)
    s = oracle.spmv(A, x)
    gx = guarded(k, dt, 0xFF, DEV, "x")
    _upload(gx.t, x)
    x_bytes = gx.bytes().clone()
    for ip in (32, 64):
        va = dA.view(ip)
        for alpha, beta in _pairs(dname):
            tag = f"{what} {dname} IP={ip} alpha={alpha} beta={beta}"
            gy = guarded(m, dt, FILL_OF[ip], DEV, "y")
            if beta == 0:
                gy.t.fill_(_nan(dname))
            else:
                _upload(gy.t, y0)
            al, be = _scalar(dname, alpha), _scalar(dname, beta)
            _lib.check(h.lib.spg_spmv(h.ptr, ctypes.byref(va), ctypes.c_void_p(gx.data_ptr()), ctypes.byref(al),
                                      ctypes.byref(be), ctypes.c_void_p(gy.data_ptr())), "spg_spmv")
            torch.cuda.synchronize()
            got = gy.t.cpu().numpy()
            want = sv.axpby(alpha, s, beta, y0)
            bad = np.flatnonzero((_bits(got).reshape(m, -1) != _bits(want).reshape(m, -1)).any(axis=1))
            assert bad.size == 0, f"{tag}: {bad.size} rows differ, first {bad[:8]}, lengths {np.diff(A.indptr)[bad[:8]]}"
            gy.check(tag + " y")
            gx.check(tag + " x")
            assert torch.equal(gx.bytes(), x_bytes), f"{tag}: x changed"


@pytest.mark.parametrize("dname", DNAMES)
def test_spmv_seam_matrix(dname):
    _spmv_case(ds.seam_matrix(ds.SPMV_CH, dname), dname, "seam_matrix(1024)")


@pytest.mark.parametrize("rows", ds.ROW_COUNTS)
@pytest.mark.parametrize("dname", DNAMES)
def test_spmv_row_counts(dname, rows):
    _spmv_case(ds.row_count_matrix(rows, dname), dname, f"{rows} rows")


def _spmm_case(A, dname, n, order, ldb, ldc, ip, what):
    """One guarded B, then the four (alpha, beta) pairs into fresh guarded C's.  Row-major: B is
    k x ldb, C is m x ldc; column-major: B is n x ldb, C is n x ldc (the transposes' rows)."""
    from spmm_amd import _lib
    dt = inst.DTYPES[dname]
    m, k = A.shape
    h = _handle()
    dA = inst.Uploaded(A, DEV)
    va = dA.view(ip)
    vt = inst.VALUE_TYPE[dname]
    row = order == _lib.SPG_ORDER_ROW
    B = ds.dense_values("B", (k, n), dt)
    C0 = ds.dense_values("C0", (m, n), dt)
    S = oracle.spmm(A, B)
    fill = FILL_OF[ip]
    gb = guarded((k, ldb) if row else (n, ldb), dt, fill, DEV, "B")
    _upload(gb.t[:, :n] if row else gb.t[:, :k], B if row else B.T)
    b_bytes = gb.bytes().clone()
    vb = _lib.SpgDense(k, n, ldb, gb.data_ptr(), order, vt)
    for alpha, beta in _pairs(dname):
        tag = f"{what} {dname} n={n} IP={ip} ldb={ldb} ldc={ldc} alpha={alpha} beta={beta}"
        gc = guarded((m, ldc) if row else (n, ldc), dt, fill, DEV, "C")
        inner = gc.t[:, :n] if row else gc.t[:, :m]
        if beta == 0:
            inner.fill_(_nan(dname))
        else:
            _upload(inner, C0 if row else C0.T)
        vc = _lib.SpgDense(m, n, ldc, gc.data_ptr(), order, vt)
        al, be = _scalar(dname, alpha), _scalar(dname, beta)
        _lib.check(h.lib.spg_spmm(h.ptr, ctypes.byref(va), ctypes.byref(vb), ctypes.byref(al), ctypes.byref(be),
                                  ctypes.byref(vc)), "spg_spmm")
        torch.cuda.synchronize()
        got = inner.cpu().numpy()
        got = got if row else got.T
        want = sv.axpby(alpha, S, beta, C0)
        bad = np.argwhere((_bits(got).reshape(m, n, -1) != _bits(want).reshape(m, n, -1)).any(axis=2))
        assert bad.size == 0, f"{tag}: {len(bad)} elements differ, first (row, column) {bad[:6].tolist()}"
        _padding_intact(gc.t[:, n:] if row else gc.t[:, m:], fill, tag + " C")
        gc.check(tag + " C")
        gb.check(tag + " B")
        assert torch.equal(gb.bytes(), b_bytes), f"{tag}: B changed"


@pytest.mark.parametrize("n", [1, 9])
@pytest.mark.parametrize("dname", DNAMES)
def test_spmm_col_major_seam_matrix(dname, n):
    """n = 9: one full strip of NC columns (8, complex128: 4) plus a partial one for every type."""
    from spmm_amd import _lib
    A = ds.seam_matrix(ds.SPMM_CH, dname)
    m, k = A.shape
    for ip in (32, 64):
        _spmm_case(A, dname, n, _lib.SPG_ORDER_COL, k + 3, m + 3, ip, "seam_matrix(512) column-major")


@pytest.mark.parametrize("n", [4, 5, 8, 9, 16, 31, 32, 33])
@pytest.mark.parametrize("dname", DNAMES)
def test_spmm_row_major_lengths(dname, n):
    """Leading dimensions that allow 16-byte accesses (a multiple of 16 bytes; the guarded bases
    are 256-byte aligned) and ones that force the scalar kernels."""
    from spmm_amd import _lib
    A = ds.row_major_matrix(dname)
    vmax = 16 // np.dtype(inst.DTYPES[dname]).itemsize
    aligned = -(-n // vmax) * vmax
    for ip in (32, 64):
        for ld in (aligned, aligned + 1):
            _spmm_case(A, dname, n, _lib.SPG_ORDER_ROW, ld, ld, ip, "row-major lengths")
